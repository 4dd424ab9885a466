"""GPU: the four tables of the genomic index (suffix array, LCP array, 8-mer interval table) and the index file.
Every table the device build makes is read back through the file pgpu_index_save writes (it holds them verbatim,
tests/index_file_lib.py) and compared, exactly, with the CPU oracle and the text; the loader must keep all of them
and must refuse every damaged file.

A damaged file that is accepted is destroyed at once and fails the test: no pairing, find or DP job ever runs on it."""
import ctypes as C
import gzip
import os
import stat

import numpy as np
import pytest

import index_file_lib as IF

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check_built_and_reloaded(ctx, name, gen, tmp_path):
    import pintron_amd.capi as capi
    first, second = str(tmp_path / (name + ".idx")), str(tmp_path / (name + ".again.idx"))
    built = capi.Index(ctx, gen)
    try:
        built.save(first)
    finally:
        built.close()
    header, arrays = IF.parse(first)
    sa, lcp = IF.expected_sa_lcp(gen)
    assert np.array_equal(arrays["sa"], sa), (name, "suffix array")
    assert np.array_equal(arrays["lcp"], lcp), (name, "LCP", np.nonzero(arrays["lcp"] != lcp)[0][:5].tolist())
    IF.check_kmer_table(arrays["klo"], arrays["khi"], IF.expected_kmer_table(gen, sa), name)
    assert (header["len"], header["ktab"], header["version"]) == (len(gen), IF.KTAB, IF.VERSION), name
    assert header["hash"] == IF.fnv1a64(gen), name
    assert header["payload_hash"] == IF.payload_hash(arrays), name
    # the loaded index holds the same four tables: its own file is the same file
    loaded = capi.Index(ctx, gen, load_from=first)
    try:
        loaded.save(second)
    finally:
        loaded.close()
    with open(first, "rb") as a, open(second, "rb") as b:
        assert a.read() == b.read(), (name, "the file of the reloaded index differs")


@pytest.mark.parametrize("group", IF.GROUPS)
def test_tables_of_the_built_and_of_the_reloaded_index(gpu_ctx, tmp_path, group):
    cases = [c for c in IF.CASES if c[0] == group]
    assert cases
    for _, name, gen in cases:
        _check_built_and_reloaded(gpu_ctx, name, gen, tmp_path)


def test_save_replaces_a_file_and_leaves_nothing_else(gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    d = tmp_path / "cache"
    d.mkdir()
    path = d / "gene.idx"
    path.write_bytes(b"something else of another length")
    gen = IF.refusal_sequence()
    idx = capi.Index(gpu_ctx, gen)
    try:
        old = os.umask(0o077)              # the mode is set by the save, whatever the process's mask
        try:
            idx.save(str(path))
        finally:
            os.umask(old)
        header, arrays = IF.expected_file(gen)
        assert path.read_bytes() == IF.to_bytes(header, arrays)
        assert stat.S_IMODE(os.stat(path).st_mode) == 0o644
        idx.save(str(path))                # ... and over a good file
        assert path.read_bytes() == IF.to_bytes(header, arrays)
        assert os.listdir(d) == ["gene.idx"]
        missing = tmp_path / "no-such-directory"
        with pytest.raises(capi.PgpuError):
            idx.save(str(missing / "gene.idx"))
        assert not missing.exists() and sorted(os.listdir(tmp_path)) == ["cache"]
    finally:
        idx.close()


def test_the_committed_file_of_version_2_loads_and_is_written_again(gpu_ctx, tmp_path):
    """tests/golden/index_v2_n200.idx.gz: a change of the layout has to come with a new INDEX_VERSION."""
    import pintron_amd.capi as capi
    raw = gzip.open(os.path.join(GOLD, "index_v2_n200.idx.gz")).read()
    seq = open(os.path.join(GOLD, "index_v2_n200.seq"), "rb").read()
    src, again, fresh = tmp_path / "v2.idx", tmp_path / "v2.again.idx", tmp_path / "v2.fresh.idx"
    src.write_bytes(raw)
    loaded = capi.Index(gpu_ctx, seq, load_from=str(src))
    try:
        loaded.save(str(again))
    finally:
        loaded.close()
    assert again.read_bytes() == raw
    built = capi.Index(gpu_ctx, seq)
    try:
        built.save(str(fresh))
    finally:
        built.close()
    assert fresh.read_bytes() == raw


# ---- refusals -----------------------------------------------------------------------------------------------------

def _flip(words, i, bit=0):
    out = words.copy()
    out[i] ^= np.uint32(1 << bit)
    return out


def _damaged_files(gen, header, arrays):
    """[(name, bytes, rehashed)]: every way the issue lists of breaking the good file of `gen`"""
    n = len(gen)
    good = IF.to_bytes(header, arrays)
    out = [("empty", b""), ("39-bytes", good[:39]), ("header-alone", good[:40]), ("last-byte-cut", good[:-1]),
           ("last-4-bytes-cut", good[:-4]), ("cut-inside-lcp", good[:40 + 4 * n + 4 * (n // 2) + 2]),
           ("one-byte-appended", good + b"\0"), ("magic", good[:7] + b"2" + good[8:])]

    def with_header(**kw):
        return IF.to_bytes(dict(header, **kw), arrays)

    out += [("version-1", with_header(version=1)), ("version-3", with_header(version=3)), ("ktab-7", with_header(ktab=7)),
            ("len-minus-1", with_header(len=n - 1)), ("len-plus-1", with_header(len=n + 1)),
            ("hash-bit", with_header(hash=header["hash"] ^ 1)),
            ("payload-hash-bit", with_header(payload_hash=header["payload_hash"] ^ (1 << 63)))]
    for t in IF.TABLES:
        for where, i in (("first", 0), ("last", len(arrays[t]) - 1)):
            out.append(("%s-%s-word-bit" % (t, where), IF.to_bytes(header, dict(arrays, **{t: _flip(arrays[t], i)}))))
    out = [(name, data, False) for name, data in out]

    present = np.nonzero(arrays["khi"] > arrays["klo"])[0]
    absent = np.nonzero(arrays["khi"] == arrays["klo"])[0]

    def poked(table, i, value):
        a = dict(arrays)
        a[table] = arrays[table].copy()
        a[table][i] = value
        return IF.to_bytes(dict(header, payload_hash=IF.payload_hash(a)), a)

    out += [(name, data, True) for name, data in (
        ("rehashed-sa[0]=n", poked("sa", 0, n)), ("rehashed-sa[n-1]=ffffffff", poked("sa", n - 1, 0xFFFFFFFF)),
        ("rehashed-lcp[1]=n+1", poked("lcp", 1, n + 1)), ("rehashed-klo[present]=n+1", poked("klo", present[0], n + 1)),
        ("rehashed-khi[absent]=n+1", poked("khi", absent[0], n + 1)))]
    return out


def _load(ctx, path, gen):
    """(rc, handle or None) of pgpu_index_load as it is; `out` starts from a value the call has to clear"""
    out = C.c_void_p(1)
    rc = ctx.L.pgpu_index_load(ctx.h, os.fsencode(str(path)), gen, len(gen), C.byref(out))
    return rc, out.value


def _refused(ctx, path, gen, what):
    import pintron_amd.capi as capi
    rc, handle = _load(ctx, path, gen)
    if rc == capi.PGPU_OK:                          # never used: destroyed, and the test fails
        ctx.L.pgpu_index_destroy(ctx.h, handle)
        pytest.fail("pgpu_index_load accepted a damaged file: " + what)
    assert rc == capi.PGPU_EINVAL and handle is None, (what, rc, handle)


def test_every_damaged_file_is_refused(gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    gen = IF.refusal_sequence()
    good = tmp_path / "good.idx"
    idx = capi.Index(gpu_ctx, gen)
    try:
        idx.save(str(good))
    finally:
        idx.close()
    pristine = good.read_bytes()
    header, arrays = IF.parse(str(good))
    assert IF.to_bytes(header, arrays) == pristine and header["payload_hash"] == IF.payload_hash(arrays)
    damaged = _damaged_files(gen, header, arrays)
    assert len(damaged) == 15 + 8 + 5 and len({d[0] for d in damaged}) == len(damaged)
    for name, data, rehashed in damaged:
        assert data != pristine, name
        if rehashed:                                # only the range checks stand between this file and the device
            h = dict(zip(IF.HEADER_FIELDS, IF.HEADER.unpack_from(data)))
            assert h["payload_hash"] == IF.words_hash(np.frombuffer(data, dtype="<u4", offset=40)), name
            assert dict(h, payload_hash=0) == dict(header, payload_hash=0), name
        path = tmp_path / "damaged.idx"
        path.write_bytes(data)
        _refused(gpu_ctx, path, gen, name)
    # the good file, offered with another sequence
    other = bytearray(gen)
    other[150] = ord("A") if gen[150:151] != b"A" else ord("C")
    _refused(gpu_ctx, good, bytes(other), "a sequence that differs in one base")
    _refused(gpu_ctx, good, gen[:-1], "a sequence one base shorter")
    _refused(gpu_ctx, tmp_path / "missing.idx", gen, "no file")
    # ... and after all that the context still loads the untouched file, tables and all
    assert good.read_bytes() == pristine
    loaded = capi.Index(gpu_ctx, gen, load_from=str(good))
    try:
        loaded.save(str(tmp_path / "again.idx"))
    finally:
        loaded.close()
    assert (tmp_path / "again.idx").read_bytes() == pristine
