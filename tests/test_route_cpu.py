"""The routing restatement (tests/route_lib.py) and its probe set, without a GPU: the probes cover the 22 cells,
route_of agrees with every probe's literal cell, the oracle's work on them is small, and the constants the restatement
rests on are the ones in the sources."""
import os
import re

import dp_cases as D
import route_lib as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pintron_amd", "csrc")


def _text(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _const(text, name):
    """value of `constexpr <type> NAME = <products of integers>;` / `#define NAME <integer>`"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9ulUL\s*]+);" % name, text) or \
        re.search(r"#define\s+%s\s+\(?([0-9ulUL\s*<]+)\)?" % name, text)
    assert m, "constant %s not found in the sources: tests/route_lib.py has to follow them" % name
    expr = re.sub(r"[uUlL]", "", m.group(1))
    assert re.fullmatch(r"[0-9\s*<]+", expr), (name, expr)
    return eval(expr)           # digits, '*' and '<<' only


def test_probe_set_covers_the_22_cells(O):
    assert len(RL.CELLS) == 22
    scores = {id(p.case): p.case.expected(O)["score"] for p in RL.PROBES if p.case.kind == D.ALIGN}
    by_cell = {}
    for p in RL.PROBES:
        cell = RL.cell_of(p.case, RL.PROBE_INDEX_INFO, score=scores.get(id(p.case)))
        by_cell.setdefault(cell, []).append(p)
    assert sorted(by_cell) == sorted(RL.CELLS)
    few = {c: len(v) for c, v in by_cell.items() if len(v) < 3}
    assert not few, "cells with fewer than three probes: %r" % few


def test_route_of_agrees_with_every_literal_cell(O):
    bad = []
    for p in RL.PROBES:
        assert p.cell in RL.CELLS, p
        score = p.case.expected(O)["score"] if p.case.kind == D.ALIGN else None
        got = RL.cell_of(p.case, RL.PROBE_INDEX_INFO, score=score)
        if got != p.cell:
            bad.append((p, got))
    assert not bad, bad
    # the literal of a resident probe rests on the index: without one the same job is an ordinary LCF
    for p in RL.probes_of("lcf_sa/batch"):
        assert RL.route_of(p.case, None)[0] in ("lcf", "lcf_small")


def test_probe_plans_census_as_stated():
    """what expected_groups says of the plans the GPU tests build from the probes"""
    ii = RL.PROBE_INDEX_INFO
    e = RL.expected_groups(RL.probe_cases(), ii)
    assert [n for n, _ in e["groups"]] == RL.ROUTE_NAMES + [RL.BATCH]      # every route, in the table's order
    n_coop = len(RL.probes_of("borders_coop/batch")) + len(RL.probes_of("borders_coop/own"))
    assert dict(e["groups"])["borders_coop"] == n_coop and e["batched"]["borders_coop"] == 0   # 3904 rows in the plan
    assert e["dp_batch"] == sum(e["batched"].values()) == len(RL.PROBES) - sum(j for n, j in e["groups"] if n != RL.BATCH)
    for cell in RL.CELLS:
        name, form = cell.split("/")
        e = RL.expected_groups(RL.probe_cases(cell), ii)
        n = len(RL.probes_of(cell))
        own = n if form == "own" else 0
        assert e["groups"] == [(name, own)] + ([(RL.BATCH, n)] if not own else []), cell
    # the keyed route is cut every 65535 jobs
    c = RL.probe_cases("lcf/own")[0]
    assert RL.expected_groups([c] * 65535)["groups"] == [("lcf", 65535)]
    assert RL.expected_groups([c] * 65536)["groups"] == [("lcf", 65535), ("lcf", 1)]
    assert RL.expected_groups([c] * 66000)["groups"] == [("lcf", 65535), ("lcf", 465)]


def test_oracle_work_on_the_probe_set_is_bounded(O):
    """The GPU tests compute the oracle's answer to every probe once per run.  Its work is matrix cells: the whole
    set stays below 2 * 10^8 of them, and no probe needs more than the 2 * 4097 * 4300 cells of a cooperative
    BORDERS pattern at its last row count."""
    cells = [RL.oracle_cells(p.case) for p in RL.PROBES]
    assert max(cells) <= 2 * 4097 * 4300, RL.PROBES[cells.index(max(cells))]
    assert sum(cells) < 2 * 10 ** 8, sum(cells)
    for p in RL.PROBES:
        assert p.case.expected(O) is not None


def test_borders_coop_boundary_follows_from_the_sources():
    kern, internal = _text("pintron_amd", "csrc", "pgpu_dp_kernels.hip"), _text("pintron_amd", "csrc", "pgpu_internal.h")
    coop_w, max_lds = _const(kern, "COOP_W"), _const(internal, "DP_BATCH_MAX_LDS")
    assert (coop_w, max_lds) == (RL.COOP_W, RL.DP_BATCH_MAX_LDS), \
        "COOP_W / DP_BATCH_MAX_LDS changed (%d, %d): move tests/route_lib.py and its borders_coop probes" % (coop_w, max_lds)
    lds = lambda rows: (2 * (coop_w - 1) * 128 + 4 * (rows + 1)) * 4      # noqa: E731
    last = max(r for r in range(65, 4097) if lds(r) <= max_lds)
    assert last == RL.BORDERS_COOP_LAST_IN_BATCH == 3903
    assert RL.borders_coop_lds(last) == 65536 and RL.borders_coop_lds(last + 1) == 65552
    rows = sorted(len(p.case.a) for p in RL.PROBES if p.cell.startswith("borders_coop/"))
    assert {last - 1, last, last + 1, last + 2} <= set(rows)
    for p in RL.PROBES:
        if p.cell.startswith("borders_coop/"):
            assert (len(p.case.a) <= last) == (p.cell == "borders_coop/batch"), p


def test_routing_constants_follow_from_the_sources():
    """the numeric constants the restatement repeats; the thresholds classify and ROUTES[] spell out in code are
    checked where they act, by the census of tests/test_gpu_routes.py"""
    internal, header = _text("pintron_amd", "csrc", "pgpu_internal.h"), _text("include", "pintron_gpu.h")
    assert _const(internal, "ALIGN_BAND_HALF") == RL.ALIGN_BAND_HALF
    assert _const(internal, "ROW_CLASS_STRIPS") == RL.ROW_CLASS_STRIPS
    assert (_const(header, "PGPU_MAX_ROWS_LEV"), _const(header, "PGPU_MAX_ROWS_GAP"), _const(header, "PGPU_MAX_GAP_SIDE"),
            _const(header, "PGPU_MAX_GAP_CELLS"), _const(header, "PGPU_MAX_COLS")) == \
        (RL.MAX_ROWS_LEV, RL.MAX_ROWS_GAP, RL.MAX_GAP_SIDE, RL.MAX_GAP_CELLS, RL.MAX_COLS)


def test_row_class_edges():
    assert [RL.row_class(n) for n in (0, 1, 64, 65, 128, 129, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097)] == \
        [1, 1, 1, 2, 2, 4, 4, 8, 16, 32, 32, 64, 64, 128]
