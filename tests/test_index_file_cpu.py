"""The index-file restatement (tests/index_file_lib.py) without a GPU: the oracle's suffix array and LCP array against
a brute-force sort and scan, the expected 8-mer table against a scan of every text position, the restated constants
against the sources, and layout and checksums against the committed file of format version 2."""
import gzip
import os
import random
import re

import numpy as np
import pytest

import index_file_lib as IF
import pairing_lib as PL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "index_v2_n200.idx.gz")
FIXTURE_SEQ = os.path.join(HERE, "golden", "index_v2_n200.seq")


def _text(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _common_prefix(a: bytes, b: bytes) -> int:
    k = 0
    while k < len(a) and k < len(b) and a[k] == b[k]:
        k += 1
    return k


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 33, 200])
def test_oracle_suffix_array_and_lcp_vs_brute_force(O, n):
    rng = random.Random(50 + n)
    g = bytes(rng.choice(b"ACN") for _ in range(n))
    oi = PL.OracleIndex(g)
    sa, lcp = oi.sa(), oi.lcp()
    oi.close()
    want = sorted(range(n), key=lambda i: g[i:])
    assert sa.tolist() == want
    want_lcp = [0] + [_common_prefix(g[want[k - 1]:], g[want[k]:]) for k in range(1, n)] + ([0] if n else [])
    assert lcp.tolist() == want_lcp and len(lcp) == n + 1


def _kmer_table_by_text_scan(g: bytes, sa):
    """{8-mer code: sorted suffix-array slots of its occurrences}, from the text positions"""
    slot_of = {int(t): k for k, t in enumerate(sa)}
    by_code = {}
    for i in range(len(g) - 7):
        w = g[i:i + 8]
        if all(c in b"ACGT" for c in w):
            code = 0
            for c in w:
                code = code * 4 + b"ACGT".index(c)
            by_code.setdefault(code, []).append(slot_of[i])
    return {c: sorted(v) for c, v in by_code.items()}


@pytest.mark.parametrize("name", ["AC-periodic", "last-8-repeated", "one-N-one-lower-one-star"])
def test_expected_kmer_table_vs_text_scan(O, name):
    g = b"AC" * 40 + b"ACGTTGCA" + b"N" + b"ACGTTGCA" if name == "AC-periodic" else \
        next(c[2] for c in IF.CASES if c[1] == name)
    sa, _ = IF.expected_sa_lcp(g)
    klo, khi, present = IF.expected_kmer_table(g, sa)
    scan = _kmer_table_by_text_scan(g, sa)
    assert len(scan) > 1 and sorted(scan) == np.nonzero(present)[0].tolist()
    for code, slots in scan.items():
        assert slots == list(range(int(klo[code]), int(khi[code]))), code
    assert not klo[~present].any() and not khi[~present].any()
    if name == "last-8-repeated":             # the suffix of exactly 8 characters is in its 8-mer's interval
        code = int(IF.kmer_codes(g)[len(g) - 8])
        assert code >= 0 and khi[code] - klo[code] >= 2 and (len(g) - 8) in sa[klo[code]:khi[code]]
    if name == "one-N-one-lower-one-star":    # no window over position 100, 300 or 500 has a code
        codes = IF.kmer_codes(g)
        for p in (100, 300, 500):
            assert (codes[p - 7:p + 1] == -1).all() and codes[p - 8] >= 0 and codes[p + 1] >= 0


def test_a_suffix_shorter_than_eight_is_in_no_interval(O):
    g = next(c[2] for c in IF.CASES if c[1] == "last-7-prefix")
    sa, _ = IF.expected_sa_lcp(g)
    klo, khi, present = IF.expected_kmer_table(g, sa)
    assert g[-7:] == g[200:207] and present[int(IF.kmer_codes(g)[200])]
    for t in range(len(g) - 7, len(g)):
        slot = sa.tolist().index(t)
        assert not ((klo[present] <= slot) & (slot < khi[present])).any(), t
    assert int(khi.astype(np.int64).sum() - klo.astype(np.int64).sum()) == len(g) - 7


def test_cases_are_the_listed_ones():
    by_group = {}
    for group, name, g in IF.CASES:
        by_group.setdefault(group, []).append(len(g))
    assert by_group["lengths"] == [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513]
    assert by_group["periodic"] == [4096, 4097, 8192, 8193, 10946]
    assert by_group["repeat"] == [7001] and by_group["alphabet"] == [65537]
    assert by_group["kmer-edges"] == [1000, 1000, 600]
    assert len({name for _, name, _ in IF.CASES}) == len(IF.CASES)
    assert set(next(c[2] for c in IF.CASES if c[0] == "alphabet")) == set(IF.ALPHABET)


def test_restated_constants_are_the_sources():
    src = _text("pintron_amd", "csrc", "pgpu_index.hip")
    m = re.search(r"INDEX_MAGIC\[8\]\s*=\s*\{([^}]*)\}", src)
    assert m and bytes(ord(c) for c in re.findall(r"'(.)'", m.group(1))) == IF.MAGIC
    m = re.search(r"constexpr\s+uint32_t\s+INDEX_VERSION\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == IF.VERSION
    m = re.search(r"struct\s+IndexFileHeader\s*\{([^}]*)\}", src)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, nm.strip()) for nm in names.split(",")]
    assert fields == [("char", "magic[8]"), ("uint32_t", "version"), ("uint32_t", "ktab"), ("uint64_t", "len"),
                      ("uint64_t", "hash"), ("uint64_t", "payload_hash")]
    assert [f[1].split("[")[0] for f in fields] == list(IF.HEADER_FIELDS) and IF.HEADER.size == 40
    m = re.search(r"constexpr\s+uint32_t\s+KTAB\s*=\s*(\d+)\s*;", _text("pintron_amd", "csrc", "pgpu_index.h"))
    assert m and int(m.group(1)) == IF.KTAB and IF.KTAB_ENTRIES == 65536
    # the file's payload is the four tables in this order, as the save routine copies them
    assert re.search(r"d_sa,[^;]*d_lcp,[^;]*d_klo,[^;]*d_khi,", src, re.S)


def test_hashes_known_answers():
    # FNV-1a's prime and loop; the offset basis is the sources' own (not the standard 0xcbf29ce484222325), in the
    # library and in the cache's file names (ef_sched.c) alike
    src = _text("pintron_amd", "csrc", "pgpu_index.hip") + _text("pintron_amd", "host", "ef_sched.c")
    assert src.count("%dull" % IF.FNV_BASIS) == 3 and src.count("%dull" % IF.FNV_PRIME) >= 3
    assert IF.FNV_PRIME == 0x100000001b3 and IF.fnv1a64(b"") == IF.FNV_BASIS
    assert IF.fnv1a64(b"a") == ((IF.FNV_BASIS ^ 0x61) * IF.FNV_PRIME) % 2 ** 64
    assert IF.fnv1a64(b"ab") == ((IF.fnv1a64(b"a") ^ 0x62) * IF.FNV_PRIME) % 2 ** 64
    assert IF.words_hash([]) == IF.FNV_BASIS ^ ((0x9e3779b97f4a7c15 * 0xff51afd7ed558ccd) & IF.M64)
    # an odd count: the last word goes to the first lane
    h0 = ((IF.FNV_BASIS ^ 7) * IF.FNV_PRIME) & IF.M64
    h0 = ((h0 ^ 9) * IF.FNV_PRIME) & IF.M64
    h1 = ((0x9e3779b97f4a7c15 ^ 8) * IF.FNV_PRIME) & IF.M64
    assert IF.words_hash([7, 8, 9]) == h0 ^ ((h1 * 0xff51afd7ed558ccd) & IF.M64) ^ 3


def test_fixture_layout_checksums_and_tables(O, tmp_path):
    """tests/golden/index_v2_n200.idx.gz, a file the device build wrote: parse / write reproduce it byte for byte,
    both stored checksums are the restatements over its own bytes, and its tables are the expected ones."""
    raw = gzip.open(FIXTURE).read()
    seq = open(FIXTURE_SEQ, "rb").read()
    assert len(seq) == 200 and set(seq) <= set(b"ACGT")
    path = tmp_path / "fixture.idx"
    path.write_bytes(raw)
    header, arrays = IF.parse(str(path))
    assert header["magic"] == IF.MAGIC and header["version"] == 2 and header["ktab"] == 8 and header["len"] == 200
    assert header["hash"] == IF.fnv1a64(seq)
    assert header["payload_hash"] == IF.payload_hash(arrays)
    assert header["payload_hash"] == IF.words_hash(np.frombuffer(raw, dtype="<u4", offset=40))
    assert [len(arrays[t]) for t in IF.TABLES] == [200, 201, 65536, 65536]
    again = tmp_path / "again.idx"
    IF.write(str(again), header, arrays)
    assert again.read_bytes() == raw
    sa, lcp = IF.expected_sa_lcp(seq)
    assert np.array_equal(arrays["sa"], sa) and np.array_equal(arrays["lcp"], lcp)
    IF.check_kmer_table(arrays["klo"], arrays["khi"], IF.expected_kmer_table(seq, sa), "fixture")
    e_header, e_arrays = IF.expected_file(seq)
    assert IF.to_bytes(e_header, e_arrays) == raw
