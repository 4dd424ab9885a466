"""GPU: pgpu_index_classify and pgpu_index_score5 against the reference's recorded answers
(tests/golden/classify_introns.json.gz) and, where the reference is undefined, against the CPU restatement
(tests/small_exon_lib.py) of what the product's host path does there."""
import threading

import numpy as np
import pytest

import small_exon_lib as SL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return SL.load_fixture()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_classify_equals_the_reference_on_every_triple(gpu_ctx, fixture):
    import pintron_amd.capi as capi
    for name, g, tri, _ in fixture:
        idx = capi.Index(gpu_ctx, g)
        got = idx.classify(tri[:, 0], tri[:, 1])
        idx.close()
        bad = np.nonzero(got != tri[:, 2])[0]
        assert len(bad) == 0, (name, len(bad), tri[bad[:8]].tolist(), got[bad[:8]].tolist())


def test_score5_equals_the_restatement_bit_for_bit_everywhere(gpu_ctx, fixture):
    import pintron_amd.capi as capi
    for name, g, _, sc in fixture:
        rest = SL.Classifier(g)
        idx = capi.Index(gpu_ctx, g)
        for k in range(4):
            got = idx.score5(k)
            assert got.shape == (len(g) + 1,)
            diff = np.nonzero(got.view(np.uint64) != rest.score5[k].view(np.uint64))[0]
            assert len(diff) == 0, (name, k, len(diff), diff[:5].tolist(), got[diff[:5]].tolist(), rest.score5[k][diff[:5]].tolist())
        tabs = [idx.score5(k) for k in range(4)]
        idx.close()
        for k, s, v in sc:                                   # and the reference's own recorded numbers
            assert float(tabs[k][s]).hex() == v.hex(), (name, k, s)


def undefined_cases(n, rng):
    s = [0, 1, 2, 0, 1, 2, 0, 5, 7, 100, 100, 100, n - 1, n - 1, n, n + 5, n - 5, n - 12, 0, 50]
    e = [40, 40, 40, 0, 1, 3, 2, 4, 3, 99, 50, 0, n - 1, n + 7, n + 3, n + 9, n + 1000, 0xFFFFFFFF, 0xFFFFFFFF, n]
    rs = rng.integers(0, n, 400)
    return np.array(s + rs.tolist(), dtype=np.int64), np.array(e + (rs + rng.integers(-50, 3000, 400)).tolist(), dtype=np.int64)


def test_undefined_inputs_equal_the_restatement(gpu_ctx):
    import pintron_amd.capi as capi
    rng = np.random.default_rng(5)
    g = bytearray(SL.synth_sequence({"seed": 77, "gen_len": 20000}))
    g[1000:1004] = b"RYKM"                                  # bytes no matrix has a row for
    g[2000] = ord("-")
    g[3000:3060] = b"x" * 60
    g[4000:4100] = bytes(g[4000:4100]).lower()
    g[-10:] = b"NNNNNNNNNN"
    g = bytes(g)
    n = len(g)
    rest = SL.Classifier(g)
    s, e = undefined_cases(n, rng)
    around = np.array([p + d for p in (1000, 2000, 3000, 3059, 4000) for d in range(-16, 6)], dtype=np.int64)
    s = np.concatenate([s, around, around - 35, around - 29])
    e = np.concatenate([e, around + 60, around, around])
    e = np.maximum(e, 0)
    idx = capi.Index(gpu_ctx, g)
    got = idx.classify(s, e)
    want = rest.classify_many(s, e)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), s[bad[:8]].tolist(), e[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    for k in range(4):
        assert same_bits(idx.score5(k), rest.score5[k]), k
    assert len(idx.classify([], [])) == 0                   # n == 0 is PGPU_OK
    idx.close()
    for tiny in (b"GTAG" * 16, (b"GT" + b"C" * 27 + b"AG") * 3):
        idx = capi.Index(gpu_ctx, tiny)
        r = SL.Classifier(tiny)
        ss = np.array([0, 0, 0, 1, len(tiny), 31, 31, 4], dtype=np.int64)
        ee = np.array([0, len(tiny), len(tiny) - 1, 2, 3, 61, 60, 35], dtype=np.int64)
        assert idx.classify(ss, ee).tolist() == r.classify_many(ss, ee).tolist(), tiny
        assert same_bits(idx.score5(0), r.score5[0])
        idx.close()


def test_a_loaded_index_answers_the_same(gpu_ctx, fixture, tmp_path):
    import pintron_amd.capi as capi
    name, g, tri, _ = fixture[0]
    path = str(tmp_path / "ambn.idx")
    built = capi.Index(gpu_ctx, g)
    built.save(path)                                        # before any class was asked: the file has no tables
    built.close()
    loaded = capi.Index(gpu_ctx, g, load_from=path)
    got = loaded.classify(tri[:, 0], tri[:, 1])
    assert np.array_equal(got, tri[:, 2].astype(np.uint8))
    assert same_bits(loaded.score5(3), SL.Classifier(g).score5[3])
    loaded.close()


def test_two_contexts_ask_a_fresh_index_at_once(gpu_ctx, fixture):
    import pintron_amd.capi as capi
    name, g, tri, _ = fixture[1]
    other = capi.Context(0)
    try:
        for _ in range(3):
            idx = capi.Index(gpu_ctx, g)                    # fresh: no tables yet
            out, err = {}, []
            gate = threading.Barrier(2)

            def ask(key, ctx):
                try:
                    gate.wait()
                    out[key] = idx.classify(tri[:, 0], tri[:, 1], ctx=ctx)
                except Exception as ex:                     # noqa: BLE001
                    err.append(ex)
            th = [threading.Thread(target=ask, args=("a", gpu_ctx)), threading.Thread(target=ask, args=("b", other))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not err, err
            for key in ("a", "b"):
                assert np.array_equal(out[key], tri[:, 2].astype(np.uint8)), key
            idx.close()
    finally:
        other.close()


def test_bad_arguments(gpu_ctx):
    import ctypes as C
    import pintron_amd.capi as capi
    L = capi.lib()
    idx = capi.Index(gpu_ctx, b"ACGT" * 50)
    out = (C.c_uint8 * 1)()
    assert L.pgpu_index_classify(gpu_ctx.h, idx.h, None, 1, out) == capi.PGPU_EINVAL
    iv = (capi.Intron * 1)(capi.Intron(1, 2))
    assert L.pgpu_index_classify(gpu_ctx.h, idx.h, iv, 1, None) == capi.PGPU_EINVAL
    assert L.pgpu_index_classify(gpu_ctx.h, idx.h, None, 0, None) == capi.PGPU_OK
    sc = (C.c_double * 300)()
    assert L.pgpu_index_score5(gpu_ctx.h, idx.h, 4, sc, 300) == capi.PGPU_EINVAL
    assert L.pgpu_index_score5(gpu_ctx.h, idx.h, -1, sc, 300) == capi.PGPU_EINVAL
    assert L.pgpu_index_score5(gpu_ctx.h, idx.h, 0, sc, 200) == capi.PGPU_ENOSPC
    assert L.pgpu_index_score5(gpu_ctx.h, idx.h, 0, sc, 201) == capi.PGPU_OK
    assert idx.classify([3], [40]).tolist() == SL.Classifier(b"ACGT" * 50).classify_many([3], [40]).tolist()
    idx.close()
