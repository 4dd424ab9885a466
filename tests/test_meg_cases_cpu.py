"""CPU: the inputs of tests/test_gpu_meg.py reach what they were made for.  Everything here is read off the
`@@stats` line and the texts of tests/hostcheck/meg_check (host MEG code over the pairing oracle), so a GPU test
cannot pass while its input misses the edge it is aimed at."""
import pytest

import meg_lib as M


@pytest.fixture(scope="module")
def crafted():
    gfa, efa, labels = M.crafted()
    runs = {name: M.first_attempt_megs(gfa, efa, prm)[0] for name, prm in M.CRAFTED_SETS}
    for recs in runs.values():
        assert len(recs) == len(labels)
    return labels, runs


def _one(labels, recs, label):
    at = [k for k, l in enumerate(labels) if l == label]
    assert len(at) == 1, label
    return recs[at[0]]["stats"]


def test_stats_line_is_consistent(crafted):
    labels, runs = crafted
    for name, prm in M.CRAFTED_SETS:
        for e in runs[name]:
            st = e["stats"]
            assert st["build"].v == st["pairings"] + 2
            assert st["simp"].v <= st["build"].v and st["red"].v == st["simp"].v and st["red"].e <= st["simp"].e
            if not prm["trans_red"]:
                assert st["red"] == st["simp"]
            if not prm["short_edge_comp"]:
                assert st["created"] == 0 and st["peak"] == 0 and st["end"] == st["red"]
            assert st["end"].v <= st["red"].v + st["created"]
            assert (st["clause"] in ("cmeg", "edges", "density", "tp50", "compaction")) == bool(e["complex"])
            nv = len(e["meg"].split(b"#adj#\n")[0].splitlines())
            ne = len(e["meg"].split(b"#adj#\n")[1].splitlines())
            assert (nv, ne) == (st["end"].v, st["end"].e)


def test_pairing_counts_at_the_vertex_cap(crafted):
    labels, runs = crafted
    for name, prm in (("defaults", M.DEFAULTS), ("neither", M.NEITHER), ("no-compaction", M.NO_COMPACTION)):
        for n, rule in ((61, "available"), (62, "available"), (63, "unavailable")):
            st = _one(labels, runs[name], "pairings%d" % n)
            assert st["pairings"] == n and st["created"] == 0
            assert max(st["build"].adj, st["build"].inc) <= M.MAX_DEGREE          # the vertex count alone decides
            assert M.availability(st, prm) == rule
            assert st["end"].v == n + 2                                           # 64 live vertices at 62 pairings


def test_lists_of_32_and_33(crafted):
    """With the reduction and the compaction off the rule is exact: the list length after build_edge_set decides."""
    labels, runs = crafted
    recs = runs["neither"]
    for n, rule in ((32, "available"), (33, "unavailable")):
        out, inn, both = (_one(labels, recs, "%s%d" % (w, n)) for w in ("out", "in", "both"))
        assert (out["build"].adj, inn["build"].inc) == (n, n)
        assert out["build"].inc <= 1 and inn["build"].adj <= 1                    # an out-list alone, an in-list alone
        assert (both["build"].adj, both["build"].inc) == (n, n) and both["end"].adj == n and both["end"].inc == n
        for st in (out, inn, both):
            assert st["pairings"] + 2 <= M.MAX_VERTICES
            assert M.availability(st, M.NEITHER) == rule


def test_compaction_carries_the_vertex_count_over_the_cap(crafted):
    labels, runs = crafted
    on, off = _one(labels, runs["defaults"], "compaction-over"), _one(labels, runs["no-compaction"], "compaction-over")
    assert on["pairings"] == off["pairings"] and on["pairings"] + 2 <= M.MAX_VERTICES
    assert on["pairings"] + 2 + on["created"] > M.MAX_VERTICES and on["peak"] <= M.MAX_DEGREE
    assert max(on["build"].adj, on["build"].inc) <= M.MAX_DEGREE
    assert M.availability(on, M.DEFAULTS) == "unavailable" and M.availability(off, M.NO_COMPACTION) == "available"
    assert off["created"] == 0 and off["end"].v == off["pairings"] + 2


def test_compaction_makes_and_removes_vertices(crafted):
    labels, runs = crafted
    for label in ("compaction-4", "compaction-9"):
        st = _one(labels, runs["defaults"], label)
        assert M.availability(st, M.DEFAULTS) == "available"
        assert st["created"] > 0
        assert st["end"].v < st["red"].v + st["created"]                # it removed vertices
        assert st["created"] > st["end"].v - 2                          # ... more than the old ones: some it had made itself
    made_and_kept = [e for e in runs["defaults"] if e["stats"]["created"] > 0 and e["stats"]["end"].v > 2]
    assert made_and_kept


def test_over_cap_patterns_sit_between_ordinary_ones(crafted):
    labels, runs = crafted
    n_over = 0
    for name, prm in M.CRAFTED_SETS:
        rules = [M.availability(e["stats"], prm) for e in runs[name]]
        assert "grey" not in rules
        for k, rule in enumerate(rules):
            if labels[k] == "ordinary":
                assert rule == "available" and runs[name][k]["stats"]["pairings"] >= 1
            if rule == "unavailable":
                n_over += 1
                assert 0 < k < len(rules) - 1
                assert rules[k - 1] == "available" and {labels[k - 1], labels[k + 1]} <= {"ordinary", "compaction-4"}
                assert rules[k + 1] == "available"
    assert n_over >= 12


@pytest.fixture(scope="module")
def sweep():
    """{source: (defaults' records, {set: records}, {set: params})}"""
    out = {}
    for src, (gfa, efa, exons) in M.sweep_sources().items():
        sets = M.sweep_sets(exons)
        out[src] = (M.first_attempt_megs(gfa, efa)[0], {n: M.first_attempt_megs(gfa, efa, p)[0] for n, p in sets}, dict(sets))
    return out


def test_every_parameter_is_moved_and_every_set_matters(sweep):
    base, runs, sets = sweep["c2"]
    assert 280 <= len(base) <= 310                                      # about 150 ESTs, both strands
    for field in M.DEFAULTS:
        assert any(p[field] != M.DEFAULTS[field] for p in sets.values()), field
    assert {p["min_factor_len"] for p in sets.values()} >= {12, 15, 18, 20}
    assert {p["min_intron_length"] for p in sets.values()} >= {0, 25, 60}
    exons = M.sweep_sources()["c2"][2]
    assert 0 < sets["maxintron-below-shortest"]["max_intron_length"] < M.shortest_intron(exons)
    for src, (base, runs, sets) in sweep.items():
        for name, recs in runs.items():
            assert [e["seq"] for e in recs] == [e["seq"] for e in base]
            changed = sum((a["complex"], a["meg"], a["edges"]) != (b["complex"], b["meg"], b["edges"]) for a, b in zip(recs, base))
            assert changed >= 1, (src, name)
        # max_pairings_in_MEG = 0 switches the clause off: against the limit of 6 it changes records the device answers
        off, six = runs["cmeg0-freq0.1"], runs["cmeg6"]
        assert any(a["complex"] != b["complex"] and M.availability(a["stats"], sets["cmeg6"]) == "available" for a, b in zip(off, six)), src
        # edges disappear under a maximum intron length that no intron of the gene fits
        assert sum(e["stats"]["build"].e for e in runs["maxintron-below-shortest"]) < sum(e["stats"]["build"].e for e in base)
        # the workload sources may hold grey records, within the cap of the MEG-stage test
        for name, recs in list(runs.items()) + [("defaults", base)]:
            prm = sets.get(name, M.DEFAULTS)
            grey = sum(M.availability(e["stats"], prm) == "grey" for e in recs)
            assert grey * 20 <= len(recs), (src, name, grey)


def _all_runs(crafted, sweep):
    labels, runs = crafted
    for name, prm in M.CRAFTED_SETS:
        yield prm, runs[name]
    for src, (base, sruns, sets) in sweep.items():
        yield M.DEFAULTS, base
        for name, recs in sruns.items():
            yield sets[name], recs


def test_every_clause_of_too_complex_decides_a_record(crafted, sweep):
    """... in a record the device has to answer (not one it may flag unavailable)."""
    seen = set()
    for prm, recs in _all_runs(crafted, sweep):
        for e in recs:
            if M.availability(e["stats"], prm) == "available":
                seen.add((e["stats"]["clause"], e["complex"]))
    assert seen >= {("early", 0), ("cmeg", 1), ("edges", 1), ("density", 1), ("tp50", 1), ("none", 0)}, seen


def test_texts_hold_what_the_formatter_can_get_wrong(crafted, sweep):
    negative = suffix_mixed = two_digits = big_edge_index = False
    for prm, recs in _all_runs(crafted, sweep):
        for e in recs:
            if M.availability(e["stats"], prm) != "available":
                continue
            lines = e["edges"].decode().splitlines()
            negative |= any(int(f) < 0 for ln in lines for f in ln.split()[:9])
            suffix_mixed |= any(a.endswith(" intronic") != b.endswith(" intronic") for a, b in zip(lines, lines[1:]))
            adj = e["meg"].decode().split("#adj#\n")[1].splitlines()
            two_digits |= any(int(x) >= 10 for ln in adj for x in ln.split("-"))
            big_edge_index |= any(int(ln.split("-")[0]) >= 10 and int(ln.split("-")[1]) >= 10 for ln in adj)
    assert negative and suffix_mixed and two_digits and big_edge_index


def test_degenerate_inputs():
    for n in (1, 64, 65):
        recs, _ = M.first_attempt_megs(*M.degenerate(n))
        assert len(recs) == n
        assert all(M.availability(e["stats"], M.DEFAULTS) == "available" for e in recs)
    recs, _ = M.first_attempt_megs(*M.degenerate(64))
    lens = {len(e["seq"]) for e in recs}
    assert {14, 15, 16} <= lens
    by_len = {len(e["seq"]): e for e in recs}
    assert by_len[14]["stats"]["pairings"] == 0 and by_len[15]["stats"]["pairings"] == 1 and by_len[16]["stats"]["pairings"] == 1
    assert any(e["stats"]["pairings"] == 0 and len(e["seq"]) == 120 for e in recs)          # long enough, no pairing
    assert any(set(e["seq"]) == {ord("N")} and e["stats"]["pairings"] == 0 for e in recs)
    assert sum(e["stats"]["pairings"] >= 1 and e["stats"]["end"].v >= 3 for e in recs) >= 50    # the ordinary ones
    recs65, _ = M.first_attempt_megs(*M.degenerate(65))
    assert len(recs65[64]["seq"]) == 15


def test_rerun_input_outgrows_the_first_buffer():
    """tests/test_gpu_meg.py::test_reruns_on_one_plan: with both simplifications off the records are larger than the
    output buffer that the run with the defaults allocated (its size + 1/8 + 4096); L = 16 gives other records than
    L = 15; nothing is over a cap or grey."""
    gfa, efa = M.rerun_input()
    sets = dict(d15=M.DEFAULTS, d16=M.params(min_factor_len=16), neither=M.NEITHER)
    exp = {k: M.first_attempt_megs(gfa, efa, p)[0] for k, p in sets.items()}
    for k, p in sets.items():
        assert len(exp[k]) == 60 and all(M.availability(e["stats"], p) == "available" for e in exp[k])
    small = sum(M.expected_size(e, M.DEFAULTS) for e in exp["d15"])
    large = sum(M.expected_size(e, M.NEITHER) for e in exp["neither"])
    assert large > small + small // 8 + 4096, (small, large)
    differ = sum((a["meg"], a["edges"]) != (b["meg"], b["edges"]) for a, b in zip(exp["d15"], exp["d16"]))
    assert differ >= 3
    assert any(e["stats"]["created"] > 0 for e in exp["d15"])
