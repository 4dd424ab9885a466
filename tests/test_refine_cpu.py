"""CPU: the restatement of the intron-border decision (tests/refine_lib.py) against what the reference's refine_intron
returned (tests/golden/refine_introns.json.gz, tools/make_refine_golden.py), the fixture's cover of the ten branches,
and the layout of the binding's structs against the sizes and offsets include/pintron_gpu.h states."""
import ctypes as C
import os
import re

import numpy as np

import refine_lib as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_reference_on_every_case(O):
    gen, cases = RL.load_fixture()
    assert len(cases) >= 3000
    for k, c in enumerate(cases):
        er, gr, v = RL.oracle_rows(O, c["est"], gen, c["donor"], c["acceptor"], *c["settings"][:3])
        info = {}
        got = RL.refine(c["est"], gen, er, gr, v, c["donor"], c["acceptor"], c["first"], *c["settings"], info=info)
        assert got == (RL.OK, c["refined"], c["path"], c["donor_after"], c["acceptor_after"]), (k, got, c)
        assert not info["outside"], k                       # the fixture holds only what the reference defines
        if not c["refined"]:
            assert c["donor_after"] == c["donor"] and c["acceptor_after"] == c["acceptor"], k


def test_every_path_has_its_cases():
    _, cases = RL.load_fixture()
    counts = np.bincount([c["path"] for c in cases], minlength=RL.N_PATHS)
    assert len(counts) == RL.N_PATHS and all(int(n) >= 25 for n in counts), dict(zip(RL.PATH_NAMES, counts.tolist()))
    refused = sum(1 for c in cases if c["path"] >= 5 and not c["refined"])
    assert refused >= 25, refused
    assert sum(1 for c in cases if c["first"]) >= 25 and sum(1 for c in cases if not c["first"]) >= 25
    assert sum(1 for c in cases if c["acceptor"][0] - c["donor"][1] > 1) >= 25            # an unaligned EST gap
    assert sum(1 for c in cases if c["est"] != c["est"].upper()) >= 25 and sum(1 for c in cases if b"N" in c["est"]) >= 25


def test_fixture_is_no_larger_than_the_classify_fixture():
    assert os.path.getsize(RL.FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "classify_introns.json.gz"))


def test_struct_layouts_match_the_header():
    import pintron_amd.capi as capi
    hdr = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    sizes = {name: int(n) for name, n in re.findall(r"\}\s*(pgpu_refine_query|pgpu_refine_result);\s*/\*\s*(\d+) bytes", hdr)}
    assert sizes == {"pgpu_refine_query": 96, "pgpu_refine_result": 48}
    assert re.search(r"\}\s*pgpu_factor;\s*/\*[^*]*16 bytes", hdr)
    assert C.sizeof(capi.Factor) == 16 and C.sizeof(capi.RefineQuery) == 96 and C.sizeof(capi.RefineResult) == 48
    # the offsets the header lists for the query
    m = re.search(r"offsets: (.*?)no padding anywhere", hdr, re.S)
    text = re.sub(r"[*\n]", " ", m.group(1))
    stated = {name: int(off) for name, off in re.findall(r"([a-z_]+) (\d+)", text)}
    assert len(stated) == 11, stated
    for name, off in stated.items():
        assert getattr(capi.RefineQuery, name).offset == off, name
    order = [f[0] for f in capi.RefineQuery._fields_]
    assert [getattr(capi.RefineQuery, f).offset for f in order] == [0, 8, 12, 16, 24, 28, 32, 36, 40, 44, 48, 64, 80, 84, 88, 92]
    assert [getattr(capi.RefineResult, f[0]).offset for f in capi.RefineResult._fields_] == [0, 4, 8, 12, 16, 32]
    assert np.dtype(capi.REFINE_QUERY_DTYPE).itemsize == 96 and np.dtype(capi.REFINE_RESULT_DTYPE).itemsize == 48
    for name in order:
        assert np.dtype(capi.REFINE_QUERY_DTYPE).fields[name][1] == getattr(capi.RefineQuery, name).offset
    assert (capi.REFINE_MAX_DIM, capi.REFINE_MAX_ED) == (RL.MAX_DIM, RL.MAX_ED)
    assert int(re.search(r"#define PGPU_REFINE_MAX_DIM\s+(\d+)", hdr).group(1)) == RL.MAX_DIM
    assert int(re.search(r"#define PGPU_REFINE_MAX_ED\s+(\d+)", hdr).group(1)) == RL.MAX_ED
