"""Which kernel answers each DP job, in each launch form: the census of a plan (Plan.groups()) against the plain
restatement of the routing (tests/route_lib.py), and every answer against the CPU oracle.  The same job has to give
the same answer inside the batch launch and in a launch of its own, whatever else its plan holds."""
import random

import pytest

import dp_cases as D
import route_lib as RL

pytestmark = pytest.mark.gpu

_EXPECTED = {}          # id(case) -> (case, the oracle's answer): computed once, shared by every test of the module
_FULL = {}              # the plan over the whole probe set: (answers, groups)


def expected(O, case):
    if id(case) not in _EXPECTED:
        _EXPECTED[id(case)] = (case, case.expected(O))
    return _EXPECTED[id(case)][1]


@pytest.fixture(scope="module")
def probe_index(gpu_ctx):
    import pintron_amd.capi as capi
    idx = capi.Index(gpu_ctx, RL.PROBE_GENOMIC)
    yield idx
    idx.close()


def joblist(cases):
    import pintron_amd.capi as capi
    jl = capi.JobList()
    for c in cases:
        c.add_to(jl)
    return jl


def finish(plan, kinds):
    """launch .. fetch of an open plan: (decoded answers, census = [(group name, jobs with a launch of their own)])"""
    import pintron_amd.capi as capi
    plan.launch()
    plan.sync()
    res, strings = plan.fetch()
    answers = [capi.decode(kinds[i], res[i], strings) for i in range(plan.n)]
    return answers, [(g["name"], g["jobs"]) for g in plan.groups()]


def run_plan(ctx, cases, index=None, parts=None):
    """One plan over `cases` -- from several job lists when `parts` gives their sizes."""
    import pintron_amd.capi as capi
    if parts is None:
        plan = capi.Plan(ctx, joblist(cases), index)
    else:
        assert sum(parts) == len(cases)
        cut = [sum(parts[:q]) for q in range(len(parts) + 1)]
        plan = capi.Plan.from_parts(ctx, [joblist(cases[cut[q]:cut[q + 1]]) for q in range(len(parts))], index)
    try:
        return finish(plan, [c.kind for c in cases])
    finally:
        plan.close()


def assert_oracle(O, cases, answers):
    bad = [(c, expected(O, c), got) for c, got in zip(cases, answers) if not D.check_case(c, got, O, expected=expected(O, c))]
    assert not bad, "%d/%d jobs differ; first: %r\nexpected %r\ngot      %r" % (len(bad), len(cases), *bad[0])


def assert_census(cases, census, index_info=None):
    """names present, jobs per group, and the batch launch's total: the batched count of a route is the number of
    jobs classified to it minus the jobs of its group(s) -- the ABI does not report it"""
    e = RL.expected_groups(cases, index_info)
    assert census == e["groups"], "census %r\nexpected %r" % (census, e["groups"])
    own = {}
    for name, jobs in census:
        if name != RL.BATCH:
            own[name] = own.get(name, 0) + jobs
    batched = {name: e["classified"][name] - own[name] for name in own}
    assert batched == e["batched"]
    assert sum(batched.values()) == dict(census).get(RL.BATCH, 0)


def scores_of(O, cases):
    return [expected(O, c)["score"] if c.kind == D.ALIGN else None for c in cases]


def cells_seen(O, cases, census, index_info=None):
    return RL.observed_cells(cases, [dict(name=n, jobs=j) for n, j in census], scores_of(O, cases), index_info)


def full_plan(ctx, index):
    if not _FULL:
        _FULL["answers"], _FULL["census"] = run_plan(ctx, RL.probe_cases(), index)
    return _FULL["answers"], _FULL["census"]


def test_route_census(gpu_ctx, O, probe_index):
    """Plan.groups() equals the restatement -- names, jobs per group, the batch launch's total -- for the whole probe
    set, each cell's probes alone, random cases and the edge cases; every answer equals the oracle's; and every one of
    the 22 cells is seen with a non-zero count.  The two ends of align_band share one group: that a banded job ran is
    seen in the census, which end it took is the condition `oracle score <= 31` (route_lib.cell_of)."""
    ii = RL.PROBE_INDEX_INFO
    seen = set()
    plans = [("all probes", RL.probe_cases(), probe_index, ii)]
    plans += [(cell, RL.probe_cases(cell), probe_index, ii) for cell in RL.CELLS]
    plans += [("random %d" % seed, D.random_cases(random.Random(seed), n_per_kind=20, max_len=1500), None, None) for seed in (11, 12)]
    plans += [("edge cases", D.edge_cases(), None, None)]
    for what, cases, index, info in plans:
        answers, census = full_plan(gpu_ctx, index) if what == "all probes" else run_plan(gpu_ctx, cases, index)
        assert_census(cases, census, info)
        assert_oracle(O, cases, answers)
        cells = cells_seen(O, cases, census, info)
        if what in RL.CELLS:
            assert cells == {what}, (what, cells)
        seen |= cells
    assert seen == set(RL.CELLS), "cells never observed: %r" % sorted(set(RL.CELLS) - seen)


def test_same_job_both_forms(gpu_ctx, O, probe_index):
    """Every probe of a route with two forms, three ways: in a plan of its own, in the plan over all probes, and in a
    plan whose companions change what runs beside it -- for borders_coop a pattern past the LDS switch, which takes
    the whole route out of the batch launch; for a segment route a job of the other row class, so that the route has a
    part inside and a part outside in one plan.  Same decoded answer three times, equal to the oracle's, and the census
    of each plan shows the intended form."""
    ii = RL.PROBE_INDEX_INFO
    all_cases = RL.probe_cases()
    full_answers, full_census = full_plan(gpu_ctx, probe_index)
    assert_census(all_cases, full_census, ii)
    n_coop = len(RL.probes_of("borders_coop/batch")) + len(RL.probes_of("borders_coop/own"))
    assert dict(full_census)["borders_coop"] == n_coop                 # a 3904-row pattern is in that plan
    in_batch = RL.probe_cases("borders_coop/batch")
    for route in RL.TWO_FORM:
        for form, other in (("batch", "own"), ("own", "batch")):
            for case in RL.probe_cases("%s/%s" % (route, form)):
                alone, census = run_plan(gpu_ctx, [case], probe_index)
                assert census == ([(route, 1)] if form == "own" else [(route, 0), (RL.BATCH, 1)]), (case, census)
                if route == "borders_coop" and form == "batch":
                    cases = [case, RL.probe_cases("borders_coop/own")[0]]
                    want = [(route, 2)]
                elif route == "borders_coop":
                    cases = [case] + in_batch
                    want = [(route, 1 + len(in_batch))]
                else:
                    cases = [case, RL.probe_cases("%s/%s" % (route, other))[0]]
                    want = [(route, 1), (RL.BATCH, 1)]
                mixed, census = run_plan(gpu_ctx, cases, probe_index)
                assert census == want, (case, census)
                assert_census(cases, census, ii)
                assert_oracle(O, cases, mixed)
                assert_oracle(O, [case], alone)
                assert alone[0] == mixed[0] == full_answers[all_cases.index(case)], case


def _borders_in_batch_cases():
    rng = random.Random(3903)
    last = RL.BORDERS_COOP_LAST_IN_BATCH
    cases = []
    combos = [(b"", 0), (b"A", 3), (b"GT", None), (b"", None), (b"A", 0), (b"GT", 3), (b"", 3), (b"A", None), (b"GT", 0)]
    for k, n in enumerate((1501, 2048, 2049, 3000, last - 1, last)):
        p = D.rand_seq(rng, n, 0.001)
        cut = rng.randint(0, n)
        t = D.mutate(rng, p[:cut], 0.03) + b"GT" + D.rand_seq(rng, rng.randint(0, 150)) + b"AG" + D.mutate(rng, p[cut:], 0.03)
        for q, (lo, hi) in enumerate(((0, n), (n // 3, 2 * n // 3), (n - 7, n))):
            tail, errs = combos[(3 * k + q) % len(combos)]
            cases.append(D.Case(D.BORDERS, p, t, p0=lo, p1=hi, p2=n // 10 if errs is None else errs, b_tail=tail))
    assert {(len(c.b_tail), min(c.p2, 4)) for c in cases} == {(t, e) for t in (0, 1, 2) for e in (0, 3, 4)}
    return cases


def test_borders_coop_inside_the_batch_up_to_the_lds_switch(gpu_ctx, O):
    """The cooperative BORDERS sweep as a role of the batch launch at 1501 .. 3903 rows (its LDS grows with the rows,
    3903 fills the 64 KB): full range and sub-ranges, 0 / 1 / 2 bytes behind t, max_errs 0, 3 and len / 10.  Then the
    same jobs beside one pattern of 3904 rows: all of them leave the batch launch, and answer the same."""
    cases = _borders_in_batch_cases()
    inside, census = run_plan(gpu_ctx, cases)
    assert census == [("borders_coop", 0), (RL.BATCH, len(cases))]
    assert_oracle(O, cases, inside)
    beyond = RL.probe_cases("borders_coop/own")[0]
    assert len(beyond.a) == RL.BORDERS_COOP_LAST_IN_BATCH + 1
    outside, census = run_plan(gpu_ctx, cases + [beyond])
    assert census == [("borders_coop", len(cases) + 1)]
    assert_oracle(O, cases + [beyond], outside)
    assert outside[:len(cases)] == inside


def test_banded_align_behind_other_routes(gpu_ctx, O, probe_index):
    """The banded ALIGN jobs, settled and not, in a plan that also holds GAP, ED, KBAND, LCF, BORDERS and AFFIX jobs
    inside and outside the batch launch: their slice of the job table does not start at 0, and the follow-up launch
    shares the plan with launches on the other streams.  Here no BORDERS pattern is past the LDS switch, so
    borders_coop stays a role of the batch launch beside them.  Then the same from several parts, banded jobs last."""
    ii = RL.PROBE_INDEX_INFO
    banded = RL.probe_cases("align_band/settled") + RL.probe_cases("align_band/unsettled")
    others = [p.case for p in RL.PROBES if p.cell != "borders_coop/own" and not p.cell.startswith("align_band/")]
    cases = others + banded
    e = RL.expected_groups(cases, ii)
    assert e["batched"]["borders_coop"] > 0 and e["batched"]["align_band"] == len(banded)
    assert all(j > 0 for n, j in e["groups"] if n in ("gap_wave", "lev_wave<ED>", "lev_wave<KBAND>", "lcf", "gap_slow"))
    one, census = run_plan(gpu_ctx, cases, probe_index)
    assert_census(cases, census, ii)
    assert_oracle(O, cases, one)
    assert cells_seen(O, cases, census, ii) == set(RL.CELLS) - {"borders_coop/own"}
    half = len(others) // 2
    parts, census = run_plan(gpu_ctx, cases, probe_index, parts=[half, 0, len(others) - half, len(banded)])
    assert_census(cases, census, ii)
    assert parts == one
    # the banded jobs alone: the slice starts at 0
    alone, census = run_plan(gpu_ctx, banded)
    assert census == [("align_band", 0), (RL.BATCH, len(banded))]
    assert alone == one[len(others):]


def _keyed_lcf_cases():
    """50 LCF jobs of route lcf (more than 16384 cells each) with 50 different answers: a planted factor that is far
    longer than anything two random strings share, at a place of its own"""
    rng = random.Random(65535)
    cases = []
    for i in range(50):
        s1 = D.rand_seq(rng, 260 + i)
        s2 = bytearray(D.rand_seq(rng, 64))
        k, p, q = 16 + i % 20, 2 * i + 1, i % 28
        s2[q:q + k] = s1[p:p + k]
        cases.append(D.Case(D.LCF, s1, bytes(s2)))
    return cases


@pytest.mark.parametrize("n_jobs", [66000, 65535, 65536])
def test_more_than_65535_keyed_lcf_jobs(gpu_ctx, O, n_jobs):
    """A route of keyed LCF jobs is cut into launches of at most 65535 (grid.y); the keys of the second launch follow
    the first's.  50 distinct cases in a shuffled order: a key that lands on another caller's job gives that job
    another case's answer."""
    import pintron_amd.capi as capi
    cases = _keyed_lcf_cases()
    want = [expected(O, c) for c in cases]
    assert all(RL.route_of(c) == ("lcf", 0) for c in cases)
    assert len({(w["len"], w["occ1"], w["occ2"]) for w in want}) == len(cases)
    order = [i % len(cases) for i in range(n_jobs)]
    random.Random(n_jobs).shuffle(order)
    jl = capi.JobList()
    first = [c.add_to(jl) for c in cases]                      # the operands once; every further job points at them
    for i in order[len(cases):]:
        j = jl.jobs[first[i]]
        jl.jobs.append(capi.DpJob(j.kind, j.flags, j.a_off, j.b_off, j.a_len, j.b_len, j.p0, j.p1, j.p2, j.tail))
    order[:len(cases)] = range(len(cases))
    plan = capi.Plan(gpu_ctx, jl)
    try:
        answers, census = finish(plan, [D.LCF] * n_jobs)
    finally:
        plan.close()
    assert census == RL.expected_groups([cases[i] for i in order])["groups"]
    assert census == [("lcf", 65535)] + ([("lcf", n_jobs - 65535)] if n_jobs > 65535 else [])
    bad = [(q, order[q], answers[q], want[order[q]]) for q in range(n_jobs)
           if answers[q] != dict(status=0, **want[order[q]])]
    assert not bad, (len(bad), bad[0])


def test_second_open_plan_takes_buffers_of_its_own(gpu_ctx, O, probe_index):
    """While one plan is open on a context, a second one cannot borrow the context's buffers and allocates its own
    (pgpu_dp_plan_create_parts: pooled = false).  The probe plan as the second of two open plans: the same groups and
    the same answers as alone; and the first plan, launched afterwards, still answers its own jobs."""
    import pintron_amd.capi as capi
    ii = RL.PROBE_INDEX_INFO
    all_cases = RL.probe_cases()
    alone, alone_census = full_plan(gpu_ctx, probe_index)
    first_cases = D.random_cases(random.Random(5), n_per_kind=3, max_len=200)
    first = capi.Plan(gpu_ctx, joblist(first_cases))
    try:
        second, census = run_plan(gpu_ctx, all_cases, probe_index)
        assert_census(all_cases, census, ii)
        assert census == alone_census
        assert second == alone
        assert_oracle(O, all_cases, second)
        answers, census = finish(first, [c.kind for c in first_cases])
        assert_census(first_cases, census)
        assert_oracle(O, first_cases, answers)
    finally:
        first.close()
