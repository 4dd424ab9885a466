"""CPU: the intron-class and small-exon entry points are exported, bound and documented, have the stated layouts,
reject NULL arguments without a device, and their kernels use no scratch memory, spill nothing and stay within the LDS
bound; the CPU restatement of the classification (tests/small_exon_lib.py) equals the reference's recorded answers
(tests/golden/classify_introns.json.gz) on every triple and every score, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resource_lib
import small_exon_lib as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pintron_amd", "csrc")
NEW = ["pgpu_index_classify", "pgpu_index_score5", "pgpu_index_small_exons", "pgpu_index_small_exons_kernel_ms"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    import pintron_amd.capi as capi
    return capi


def test_entry_points_are_exported_bound_and_documented(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    for nm in NEW:
        assert hasattr(L, nm), nm
        assert nm in capi.EXPORTS, nm
        assert re.search(r"\b(int|double)\s+%s\s*\(" % nm, hdr), nm
    for text in ("pgpu_intron", "pgpu_sexon_query", "pgpu_sexon_result", "PGPU_SEXON_MAX_ELEN 64",
                 "src/factorization-refinement.c:641-871", "src/classify-intron.c:95-229", ":772-834",
                 "smallest offstart"):
        assert text in hdr, text
    assert L.pgpu_abi_version() == 1                      # the change is additive
    for nm in ("classify", "score5", "small_exons"):
        assert hasattr(capi.Index, nm), nm
    assert L.pgpu_index_small_exons_kernel_ms() == 0.0
    import __graft_entry__ as g
    assert "pgpu_classify.hip" in g.HIP_SOURCES


def test_struct_layouts(capi):
    assert C.sizeof(capi.Intron) == 8 and capi.Intron.end.offset == 4
    q = capi.SexonQuery
    assert C.sizeof(q) == 40                               # 36 bytes of fields + 4 of padding (alignment of e_off)
    assert [f[0] for f in q._fields_] == ["e_off", "elen", "allgstart", "allglen", "f1slen", "f2plen", "min_intron_len", "reserved"]
    assert [getattr(q, f[0]).offset for f in q._fields_] == [0, 8, 12, 16, 20, 24, 28, 32]
    r = capi.SexonResult
    assert C.sizeof(r) == 32
    assert [f[0] for f in r._fields_] == ["status", "len", "offstart", "offend", "gpos", "i1type", "i2type", "pad"]
    assert [getattr(r, f[0]).offset for f in r._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert np.dtype(capi.SEXON_QUERY_DTYPE).itemsize == 40 and np.dtype(capi.SEXON_RESULT_DTYPE).itemsize == 32
    assert capi.SEXON_MAX_ELEN == 64
    hdr = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    assert re.search(r"4 bytes of padding", hdr) and re.search(r"pgpu_sexon_query;\s*/\* 40 bytes \*/", hdr)
    assert re.search(r"pgpu_sexon_result;\s*/\* 32 bytes \*/", hdr)


def test_null_arguments_are_einval_without_a_device(capi):
    L = capi.lib()
    iv = (capi.Intron * 1)(capi.Intron(10, 50))
    out = (C.c_uint8 * 1)()
    assert L.pgpu_index_classify(None, None, iv, 1, out) == capi.PGPU_EINVAL
    sc = (C.c_double * 4)()
    assert L.pgpu_index_score5(None, None, 0, sc, 4) == capi.PGPU_EINVAL
    q = (capi.SexonQuery * 1)(capi.SexonQuery(0, 6, 0, 100, 6, 6, 4, 0))
    r = (capi.SexonResult * 1)()
    assert L.pgpu_index_small_exons(None, None, b"ACGTAC", 6, q, 1, r) == capi.PGPU_EINVAL


def test_kernels_have_no_stack_frame_and_little_lds(tmp_path):
    assert resource_lib.hipcc(), "no hipcc here"
    usage = resource_lib.usage("pgpu_classify.hip", tmp_path)
    kernels = {k: v for k, v in usage.items() if "kernel" in k}
    for want in ("class_tables_kernel", "classify_kernel", "small_exons_kernel"):
        assert any(want in k for k in kernels), (want, sorted(usage))
    for name, u in kernels.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 16 * 1024, (name, u)


def test_device_copy_of_the_matrices_equals_the_host_file():
    """pgpu_pwm_data.h (what the library uploads products of) holds the numbers of ef_classify.c, entry by entry"""
    dev = SL.parse_pwm_file(os.path.join(CSRC, "pgpu_pwm_data.h"))
    host = SL.parse_pwm_file(os.path.join(ROOT, "pintron_amd", "host", "ef_classify.c"))
    assert len(dev) == 6 and dev == host


def test_device_code_neither_multiplies_nor_takes_logarithms():
    """the route chosen for bit-exact scores: tables from the host, ordered additions and one division on the device"""
    src = open(os.path.join(CSRC, "pgpu_classify.hip")).read()
    assert "fp contract(off)" in src and "__dadd_rn" in src and "__ddiv_rn" in src
    dev = src[src.index("__device__"):src.index("// ---- the tables of an index")]
    assert not re.search(r"\blog\s*\(", dev)


def test_fixture_is_there_and_large_enough():
    assert os.path.getsize(SL.FIXTURE) < 1 << 20
    fx = SL.load_fixture()
    assert [f[0] for f in fx] == ["ambn", "cpb2", "synth-plain", "synth-n-lower"]
    assert sum(len(f[2]) for f in fx) >= 20000
    for name, g, tri, sc in fx:
        assert set(g) <= set(b"ACGTNacgtn"), name
        assert len(sc) >= 100, name
        assert set(np.unique(tri[:, 2]).tolist()) == {0, 1, 2}, name
        lens = tri[:, 1] - tri[:, 0] + 1
        assert (lens == 29).any() and (lens == 30).any() and (tri[:, 1] == len(g) - 1).any() and (tri[:, 0] <= 5).any(), name
    assert b"N" in fx[3][1] and any(c in fx[3][1] for c in b"acgt")


def test_restatement_equals_the_reference_on_every_triple_and_score():
    for name, g, tri, sc in SL.load_fixture():
        c = SL.Classifier(g)
        got = c.classify_many(tri[:, 0], tri[:, 1])
        bad = np.nonzero(got != tri[:, 2])[0]
        assert len(bad) == 0, (name, len(bad), tri[bad[:5]].tolist(), got[bad[:5]].tolist())
        for k, s, v in sc:
            assert float(c.score5[k][s]).hex() == v.hex(), (name, k, s, float(c.score5[k][s]).hex(), v.hex())


def test_transcription_finds_a_planted_small_exon_and_respects_the_tie_rule():
    """the loop with a classify function that accepts everything: the longest pattern at the smallest offstart and the
    first occurrence wins"""
    always = lambda s, e: 1                                             # noqa: E731
    small = b"GATTACAGATTACA"
    g = b"C" * 40 + small + b"C" * 50 + small + b"C" * 40
    r = SL.search_small_exon_loop(g, small, 0, len(g), 20, 20, 4, always)
    assert r == (14, 0, 0, 40, 1, 1)
    never = lambda s, e: 2                                              # noqa: E731
    assert SL.search_small_exon_loop(g, small, 0, len(g), 20, 20, 4, never) == (0, 0, 0, 0, 0, 0)
    assert SL.search_small_exon_loop(g, small, 0, len(g), 5, 20, 4, always) == (0, 0, 0, 0, 0, 0)      # a gate
    # an EST factor with a mismatching first byte: only offstart >= 1 matches, one byte shorter
    r = SL.search_small_exon_loop(g, b"T" + small[1:], 0, len(g), 20, 20, 4, always)
    assert r == (13, 1, 0, 41, 1, 1)
