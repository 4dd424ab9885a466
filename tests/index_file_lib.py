"""The genomic index file (pgpu_index_save / pgpu_index_load, pintron_amd/csrc/pgpu_index.hip) restated for the
tests, without a GPU: its layout, its two checksums, what its four tables must hold for a given sequence (from the
CPU oracle and the text alone), and the inputs the index tests build.

Layout, all little-endian: a 40-byte header
    char magic[8] = "PGPUIDX1"; u32 version; u32 ktab; u64 len; u64 hash; u64 payload_hash
then sa[len], lcp[len + 1], klo[4^ktab], khi[4^ktab], u32 each.  `hash` is FNV-1a (64 bit) of the sequence,
`payload_hash` the word-wise mix `words_hash` of the four tables taken as one array."""
import random
import struct

import numpy as np

import pairing_lib as PL

MAGIC = b"PGPUIDX1"
VERSION = 2
KTAB = 8
KTAB_ENTRIES = 4 ** KTAB
HEADER = struct.Struct("<8sIIQQQ")
HEADER_FIELDS = ("magic", "version", "ktab", "len", "hash", "payload_hash")
TABLES = ("sa", "lcp", "klo", "khi")
M64 = (1 << 64) - 1
FNV_BASIS, FNV_PRIME = 1469598103934665603, 1099511628211


def fnv1a64(data: bytes) -> int:
    h = FNV_BASIS
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def words_hash(words) -> int:
    """Two interleaved FNV-style lanes over 32-bit words (even words in one, odd words in the other; a last
    unpaired word goes to the first), folded together with the word count."""
    w = [int(x) for x in words]
    h0, h1 = FNV_BASIS, 0x9e3779b97f4a7c15
    for i in range(0, len(w) - 1, 2):
        h0 = ((h0 ^ w[i]) * FNV_PRIME) & M64
        h1 = ((h1 ^ w[i + 1]) * FNV_PRIME) & M64
    if len(w) % 2:
        h0 = ((h0 ^ w[-1]) * FNV_PRIME) & M64
    return h0 ^ ((h1 * 0xff51afd7ed558ccd) & M64) ^ len(w)


def table_sizes(n, ktab=KTAB):
    return {"sa": n, "lcp": n + 1, "klo": 4 ** ktab, "khi": 4 ** ktab}


def payload(arrays):
    return np.concatenate([np.asarray(arrays[t], dtype="<u4") for t in TABLES])


def payload_hash(arrays) -> int:
    return words_hash(payload(arrays).tolist())


def parse(path):
    """(header dict, {"sa", "lcp", "klo", "khi"} -> uint32 array) of a whole, well-formed file; the sizes come from
    the header's `len` and `ktab`, and the file must end where they say."""
    with open(path, "rb") as f:
        raw = f.read()
    assert len(raw) >= HEADER.size, "index file %s: %d bytes, no header" % (path, len(raw))
    header = dict(zip(HEADER_FIELDS, HEADER.unpack_from(raw)))
    assert header["magic"] == MAGIC and header["ktab"] <= 12, header
    sizes = table_sizes(header["len"], header["ktab"])
    assert len(raw) == HEADER.size + 4 * sum(sizes.values()), (path, len(raw), header)
    arrays, at = {}, HEADER.size
    for t in TABLES:
        arrays[t] = np.frombuffer(raw, dtype="<u4", count=sizes[t], offset=at).astype(np.uint32)
        at += 4 * sizes[t]
    return header, arrays


def to_bytes(header, arrays) -> bytes:
    return HEADER.pack(*(header[k] for k in HEADER_FIELDS)) + payload(arrays).tobytes()


def write(path, header, arrays):
    with open(path, "wb") as f:
        f.write(to_bytes(header, arrays))


# ---- what the tables must hold, from the sequence alone ---------------------------------------------------------

def expected_sa_lcp(gen: bytes):
    """Suffix array (n entries) and LCP array (n + 1 entries, zero at both ends) of the CPU oracle: a comparison
    sort of the suffixes and Kasai's scan."""
    oi = PL.OracleIndex(gen)
    try:
        return oi.sa(), oi.lcp()
    finally:
        oi.close()


_BASE = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    _BASE[_c] = _i


def kmer_codes(gen: bytes):
    """code[i] = 2-bit code of gen[i:i+8] (A=0, C=1, G=2, T=3, first base most significant), or -1 where fewer than
    8 characters are left or one of them is not an upper-case A, C, G, T."""
    n = len(gen)
    code = np.full(n, -1, dtype=np.int64)
    if n < KTAB:
        return code
    base = _BASE[np.frombuffer(gen, dtype=np.uint8)]
    m = n - KTAB + 1
    acc, ok = np.zeros(m, dtype=np.int64), np.ones(m, dtype=bool)
    for x in range(KTAB):
        b = base[x:x + m]
        ok &= b >= 0
        acc = acc * 4 + np.where(b >= 0, b, 0)
    code[:m] = np.where(ok, acc, -1)
    return code


def expected_kmer_table(gen: bytes, sa):
    """(klo, khi, present): for every 8-mer code that heads a suffix, klo = the least suffix-array slot whose suffix
    starts with it and khi = the greatest + 1; the slots between must all be its own (asserted here: suffixes that
    share a prefix are neighbours in a correct suffix array).  present[code] is False for every other code, whose
    klo and khi are left 0 here and only have to be EQUAL in a table under test (check_kmer_table)."""
    code_at_slot = kmer_codes(gen)[np.asarray(sa, dtype=np.int64)]
    slots = np.nonzero(code_at_slot >= 0)[0]
    codes = code_at_slot[slots]
    klo = np.full(KTAB_ENTRIES, len(gen) + 1, dtype=np.int64)
    khi = np.zeros(KTAB_ENTRIES, dtype=np.int64)
    np.minimum.at(klo, codes, slots)
    np.maximum.at(khi, codes, slots + 1)
    count = np.bincount(codes, minlength=KTAB_ENTRIES)
    present = count > 0
    klo[~present] = 0
    assert np.array_equal(khi - klo, count), "the suffixes of one 8-mer are not contiguous in this suffix array"
    return klo.astype(np.uint32), khi.astype(np.uint32), present


def check_kmer_table(klo, khi, expected, what=""):
    e_lo, e_hi, present = expected
    assert np.array_equal(klo[present], e_lo[present]), (what, "klo")
    assert np.array_equal(khi[present], e_hi[present]), (what, "khi")
    assert np.array_equal(klo[~present], khi[~present]), (what, "an absent 8-mer has a non-empty interval")


def expected_file(gen: bytes):
    """(header, arrays) of the file a correct build writes for `gen` (absent 8-mers as 0 / 0, what the build's
    zero-filled tables hold)."""
    sa, lcp = expected_sa_lcp(gen)
    klo, khi, _ = expected_kmer_table(gen, sa)
    arrays = {"sa": sa, "lcp": lcp, "klo": klo, "khi": khi}
    header = {"magic": MAGIC, "version": VERSION, "ktab": KTAB, "len": len(gen), "hash": fnv1a64(gen),
              "payload_hash": payload_hash(arrays)}
    return header, arrays


# ---- inputs -----------------------------------------------------------------------------------------------------

ALPHABET = b"ACGTNacgt*#"


def _random(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _fibonacci(n):
    a, b = b"A", b"AC"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _cases():
    """[(group, name, sequence)]: the boundaries of the build (256-thread blocks, the 8-mer width, the 16 / 32-base
    packing words, powers of two where the doubling ends on `distinct == n` or on `h >= n`), the most doubling
    rounds, long LCPs, the whole alphabet, and 8-mers at the end of the text and across characters outside ACGT."""
    out = []
    for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        out.append(("lengths", "random-%d" % n, _random(random.Random(1000 + n), n)))
    out += [("periodic", "A*4096", b"A" * 4096), ("periodic", "A*4097", b"A" * 4097),
            ("periodic", "AC*4096", b"AC" * 4096), ("periodic", "ACG*2731", b"ACG" * 2731),
            ("periodic", "fibonacci-10946", _fibonacci(10946))]
    rng = random.Random(31)
    unit = _random(rng, 3000)
    out.append(("repeat", "unit-3000-twice", _random(rng, 500) + unit + b"N" + unit + _random(rng, 500)))
    out.append(("alphabet", "all-bytes-65537", _random(random.Random(32), 65537, ALPHABET)))
    rng = random.Random(33)
    g = bytearray(_random(rng, 1000))
    g[-8:] = g[100:108]                       # the last suffix of 8 characters shares its 8-mer with position 100
    out.append(("kmer-edges", "last-8-repeated", bytes(g)))
    g = bytearray(_random(rng, 1000))
    g[-7:] = g[200:207]                       # 7 characters: a prefix of an 8-mer, itself in no interval
    out.append(("kmer-edges", "last-7-prefix", bytes(g)))
    g = bytearray(_random(rng, 600))
    g[100:101], g[300:301], g[500:501] = b"N", b"a", b"*"
    out.append(("kmer-edges", "one-N-one-lower-one-star", bytes(g)))
    return out


CASES = _cases()
GROUPS = sorted({c[0] for c in CASES})
assert all(set(c[2]) <= set(ALPHABET) for c in CASES)


def refusal_sequence():
    """The 300-base sequence whose good file the refusal tests damage."""
    return _random(random.Random(34), 300)

