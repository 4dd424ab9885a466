"""CPU restatement of the text stage (pgpu_unit_texts, pgpu_pairing_plan_run_texts; the rule: include/pintron_gpu.h): from a
unit's group in the packed records to its lines of raw-multifasta-out.txt and its entry of processed-ests.txt.

texts            units (numpy, UNIT_RESULT_DTYPE), their blob, one header per unit, one sequence per pattern and the original
                 genomic sequence -> (results as a numpy array of TEXT_RESULT_DTYPE, raw, pests).  Three arguments break the
                 rule on purpose (the cases must notice): WRONG.
units_of_blob    a record blob as the program writes it -> ALIGNED pgpu_unit_results with first_byte and n_bytes, pattern i
                 for the i-th group, and the groups' est_index.
hand_cases       hand-made units; batch() lays a list of them out as one call, with units, patterns and groups in three
                 different orders; tags_of() says what a case reaches; stretches() the (source mod 4, destination mod 4,
                 length) of every stretch the copy loop moves in a laid-out batch.
program_texts    the program's records, raw-multifasta-out.txt and processed-ests.txt of one run, and per_est() to cut the
                 two files into the texts of each group.
"""
import os
import random
import struct
import subprocess

import numpy as np

import unit_lib as UL

NONE, DONE, HOST = 0, 1, 2                               # PGPU_TEXT_*
MAX_UNIT_BYTES = 1 << 24
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
WRONG = ("no_clip", "unsigned", "pattern_order")
LENGTHS = list(range(10)) + [63, 64, 65, 255, 256, 257]


def stretch(seq, a, b, clip=True):
    """the bytes of seq that the 1-based, inclusive [a, b] names"""
    if clip:
        if a < 1 or a > len(seq) + 1 or b < a:
            return b""
        return seq[a - 1:a - 1 + min(b + 1 - a, len(seq) - (a - 1))]
    # clipping left out: what lies before and behind the sequence stands in as '?', eight of them at the most
    if b < a:
        return b""
    piece = seq[max(a - 1, 0):max(b, 0)]
    return piece + b"?" * min(b + 1 - a - len(piece), 8)


def number(v, signed=True):
    return b"%d" % (v if signed else v & 0xffffffff)


def raw_of(header, facts, seq, genomic, wrong=None):
    """raw(u) of one group: facts = [(polya, polyad, [(est_start, est_end, gen_start, gen_end)])]"""
    out = []
    for polya, polyad, exons in facts:
        out.append(b">" + header + b"\n#polya=%d\n#polyad=%d\n" % (polya, polyad))
        for a, b, c, d in exons:
            out.append(b" ".join(number(v, wrong != "unsigned") for v in (a, b, c, d)) + b" " +
                       stretch(seq, a, b, wrong != "no_clip") + b" " + stretch(genomic, c, d, wrong != "no_clip") + b"\n")
    return b"".join(out)


def pests_of(header, seq):
    return b">" + header + b"\n" + seq + b"\n"


def group_facts(blob, at):
    """the factorizations of the group at blob[at:]"""
    n_fact = struct.unpack_from("<I", blob, at + 4)[0]
    pos, facts = at + 8, []
    for _ in range(n_fact):
        polya, polyad, n = struct.unpack_from("<BBH", blob, pos)
        facts.append((polya, polyad, [struct.unpack_from("<4i", blob, pos + 4 + 16 * k) for k in range(n)]))
        pos += 4 + 16 * n
    return facts, pos - at


def texts(units, blob, headers, seqs, genomic, wrong=None):
    """-> (results as a numpy array of TEXT_RESULT_DTYPE, raw, pests); wrong: None or one of WRONG"""
    from pintron_amd import capi
    assert wrong is None or wrong in WRONG
    out = np.zeros(len(units), dtype=np.dtype(capi.TEXT_RESULT_DTYPE))
    made = []
    for i in range(len(units)):
        if int(units["verdict"][i]) != UL.U_ALIGNED:
            continue
        p = int(units["pattern"][i])
        facts, n = group_facts(blob, int(units["first_byte"][i]))
        assert n == int(units["n_bytes"][i])
        raw, pests = raw_of(headers[i], facts, seqs[p], genomic, wrong), pests_of(headers[i], seqs[p])
        if len(raw) > MAX_UNIT_BYTES or len(pests) > MAX_UNIT_BYTES:
            out["verdict"][i] = HOST
            continue
        out["verdict"][i] = DONE
        made.append((p if wrong == "pattern_order" else i, i, raw, pests))
    raws, pestss, ra, pa = [], [], 0, 0
    for _, i, raw, pests in sorted(made, key=lambda m: m[:2]):
        out["raw_first"][i], out["pests_first"][i], out["raw_bytes"][i], out["pests_bytes"][i] = ra, pa, len(raw), len(pests)
        ra += len(raw)
        pa += len(pests)
        raws.append(raw)
        pestss.append(pests)
    return out, b"".join(raws), b"".join(pestss)


def units_of_blob(blob):
    """(ALIGNED units as a numpy array of UNIT_RESULT_DTYPE: pattern i for the i-th group; [est_index])"""
    from pintron_amd import capi
    walked = UL.read_blob(blob)
    u = np.zeros(len(walked), dtype=np.dtype(capi.UNIT_RESULT_DTYPE))
    for i, (at, n, _, facts) in enumerate(walked):
        assert len(facts) < 256
        u[i] = (UL.U_ALIGNED, 0, 0, len(facts), i, at, n, 0)
    return u, [w[2] for w in walked]


# ---- hand-made cases ------------------------------------------------------------------------------------------------
GL = 200000
_made = {}


def genomic():
    """200 000 seeded bases; shared, do not modify"""
    if "g" not in _made:
        _made["g"] = bytes(random.Random(77).choices(b"ACGTacgtN", k=GL))
    return _made["g"]


def _seq(rng, n):
    return bytes(rng.choices(b"ACGTN", k=n))


def hand_cases():
    """[dict(name, header, seq, verdict (a unit verdict), facts)]; shared, do not modify"""
    if "cases" in _made:
        return _made["cases"]
    rng = random.Random(2024)
    out = []

    def add(name, facts, header=None, seq=None, verdict=UL.U_ALIGNED):
        out.append(dict(name=name, header=(b"/gb=H%04d /len=%d" % (len(out), len(out))) if header is None else header,
                        seq=_seq(rng, 120) if seq is None else seq, verdict=verdict, facts=facts))

    # every source offset, destination offset and stretch length: header lengths 0-7 shift the destination, the starts
    # the two sources
    for n in LENGTHS:
        for hl in range(8):
            ex = [(1 + s, s + n, 1001 + 17 * hl + t, 1000 + 17 * hl + t + n) for s in range(4) for t in range(4)]
            add("align_len%d_hl%d" % (n, hl), [(0, 0, ex)], header=b"hdr4567"[:hl], seq=_seq(rng, 300))
    sl = 120
    # numbers of 1 to 10 digits, 0, negatives, INT_MIN and INT_MAX, in every column
    values = [0] + [int("1234567890"[:k]) for k in range(1, 11)] + [-1, -12345, INT_MIN, INT_MAX, INT_MIN + 1, -999999999]
    for col in range(4):
        ex = []
        for v in values:
            e = [5, 40, 2000, 2050]
            e[col] = v
            ex.append(tuple(e))
        add("numbers_col%d" % col, [(0, 1, ex)])
    add("numbers_extremes", [(1, 0, [(INT_MIN, INT_MAX, INT_MIN, INT_MIN), (INT_MAX, INT_MAX, INT_MAX, INT_MIN), (1, INT_MAX, GL - 99, INT_MAX)])])
    for polya, polyad in ((0, 0), (1, 0), (0, 1), (255, 255), (10, 100), (99, 9)):
        add("flags_%d_%d" % (polya, polyad), [(polya, polyad, [(1, 30, 501, 530)])])
    # clipping, on the EST and the same on the genomic sequence
    for name, a, b in (("start_0", 0, 10), ("start_neg", -1, 10), ("start_len", sl, sl + 5), ("start_len1", sl + 1, sl + 9),
                       ("start_len2", sl + 2, sl + 9), ("end_before", 30, 29), ("end_before2", 30, 3), ("end_past", 100, sl + 50),
                       ("first_byte", 1, 1), ("last_byte", sl, sl), ("whole", 1, sl), ("end_eq_start", 60, 60)):
        g = {0: 0, -1: -1, sl: GL, sl + 1: GL + 1, sl + 2: GL + 2}.get(a, a)
        h = b if b < sl else GL + (b - sl)
        add("clip_est_" + name, [(0, 0, [(a, b, 3001, 3040)])])
        add("clip_gen_" + name, [(0, 0, [(1, 40, g, h)])])
        add("clip_both_" + name, [(1, 1, [(a, b, g, h), (2, 9, 11, 19)])])
    add("group_of_8_bytes", [])
    add("no_exons", [(1, 0, [])])
    add("no_exons_between", [(0, 0, [(1, 20, 101, 120)]), (0, 1, []), (1, 1, [(21, 40, 301, 320)])])
    for n in (1, 63, 64, 65, 128):
        add("exons_%d" % n, [(n & 1, 0, [(1 + k % 90, 1 + k % 90 + (k * 7) % 31, 4001 + 50 * k, 4001 + 50 * k + (k * 5) % 43) for k in range(n)])])
    add("two_factorizations", [(0, 0, [(1, 50, 101, 150), (51, 120, 401, 470)]), (1, 1, [(1, 60, 101, 160)])])
    add("three_factorizations", [(0, 1, [(1, 50, 101, 150)]), (1, 0, [(k * 2 + 1, k * 2 + 3, 9001 + k, 9003 + k) for k in range(70)]),
                                 (7, 7, [(3, 4, 5, 6)])])
    add("empty_header", [(0, 0, [(1, 33, 601, 633)])], header=b"")
    add("header_of_odd_bytes", [(0, 0, [(1, 33, 601, 633)])], header=bytes([0, 255, 10, 62, 35, 0, 128]) + b"tail")
    add("sequence_of_0", [(0, 0, [(1, 1, 701, 701), (0, 0, 1, 2)])], seq=b"")
    add("sequence_of_1", [(0, 0, [(1, 1, 701, 701), (1, 5, 1, 2), (2, 2, 3, 3)])], seq=b"G")
    add("sequence_of_0_group_of_8", [], seq=b"", header=b"")
    # units that are not ALIGNED between DONE neighbours
    add("unaligned_between", None, verdict=UL.U_UNALIGNED)
    add("done_neighbour_1", [(0, 0, [(1, 60, 101, 160)])])
    add("host_between", None, verdict=UL.U_HOST)
    add("done_neighbour_2", [(0, 0, [(1, 60, 101, 160)])])
    _made["cases"] = out
    return out


def cap_cases():
    """the cap on a unit's bytes: raw(u) of exactly 2^24 bytes (DONE), a byte over (HOST), pests(u) alone past it (HOST),
    with DONE neighbours.  Exons that span the 200 000 bases; the header length tunes the count."""
    if "cap" in _made:
        return _made["cap"]
    full = (1, 1, 1, GL)
    line = len(b"1 1 1 %d " % GL) + 1 + 1 + GL + 1
    n_full = (MAX_UNIT_BYTES - 64) // line
    rest = MAX_UNIT_BYTES - n_full * line                # for the factorization's header and a last, shorter line
    g = rest - 100
    last = len(b"1 1 1 %d " % g) + 1 + 1 + g + 1
    hl = rest - last - len(b">\n#polya=0\n#polyad=0\n")
    assert 0 < hl < 100
    facts = [(0, 0, [full] * n_full + [(1, 1, 1, g)])]
    seq = b"ACGTTGCA" * 10
    out = [dict(name="cap_neighbour_1", header=b"n1", seq=seq, verdict=UL.U_ALIGNED, facts=[(0, 0, [(1, 9, 1, 9)])]),
           dict(name="cap_exact", header=b"h" * hl, seq=seq, verdict=UL.U_ALIGNED, facts=facts),
           dict(name="cap_one_over", header=b"h" * (hl + 1), seq=seq, verdict=UL.U_ALIGNED, facts=facts),
           dict(name="cap_neighbour_2", header=b"n2", seq=seq, verdict=UL.U_ALIGNED, facts=[(1, 0, [(2, 8, 3, 7)])]),
           dict(name="cap_pests_alone", header=b"abc", seq=b"ACGT" * (MAX_UNIT_BYTES // 4), verdict=UL.U_ALIGNED, facts=[]),
           dict(name="cap_pests_exact", header=b"abc", seq=b"TGCA" * (MAX_UNIT_BYTES // 4 - 2) + b"AC", verdict=UL.U_ALIGNED,
                facts=[(0, 0, [(MAX_UNIT_BYTES - 8, MAX_UNIT_BYTES, 5, 5)])]),
           dict(name="cap_neighbour_3", header=b"n3", seq=seq, verdict=UL.U_ALIGNED, facts=[(1, 1, [(1, 80, GL - 3, GL + 3)])])]
    _made["cap"] = out
    return out


def group_bytes(est_index, facts):
    out = struct.pack("<II", est_index, len(facts))
    for polya, polyad, exons in facts:
        out += struct.pack("<BBH", polya, polyad, len(exons))
        for e in exons:
            out += struct.pack("<4i", *e)
    return out


def batch(cases, seed=3, shuffle=True):
    """cases -> (units, blob, headers, seqs) as the entries take them: the patterns in a seeded order of their own and the
    groups in the blob in another, so that units, patterns and groups are in three different orders (a unit that is not
    ALIGNED still has a pattern, and a header)"""
    from pintron_amd import capi
    n = len(cases)
    pat_order, grp_order = list(range(n)), list(range(n))
    if shuffle:
        random.Random(seed).shuffle(pat_order)
        random.Random(seed + 1).shuffle(grp_order)
    pattern_of = {i: k for k, i in enumerate(pat_order)}
    seqs = [cases[i]["seq"] for i in pat_order]
    units = np.zeros(n, dtype=np.dtype(capi.UNIT_RESULT_DTYPE))
    blob = bytearray(b"\xee" * 12 if shuffle else b"")                     # the first group does not begin the blob
    for i in grp_order:
        c = cases[i]
        if c["verdict"] != UL.U_ALIGNED:
            units[i] = (c["verdict"], 0, 0, 0, pattern_of[i], 0, 0, 0)
            continue
        g = group_bytes(1000 + i, c["facts"])
        units[i] = (UL.U_ALIGNED, i & 1, 0, min(len(c["facts"]), 255), pattern_of[i], len(blob), len(g), 0)
        blob += g
    return units, bytes(blob), [c["header"] for c in cases], seqs


def stretches(units, blob, headers, seqs, want):
    """{(source offset mod 4, destination offset mod 4, length)} of every E and X stretch of the DONE units of a laid-out
    batch, as the form without a plan places them (every array at a multiple of 256, the sequences one behind the other)"""
    seq_at = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    seen = set()
    for i in range(len(units)):
        if int(want["verdict"][i]) != DONE:
            continue
        p = int(units["pattern"][i])
        facts, _ = group_facts(blob, int(units["first_byte"][i]))
        at = int(want["raw_first"][i])
        for polya, polyad, exons in facts:
            at += len(headers[i]) + len(b">\n#polya=%d\n#polyad=%d\n" % (polya, polyad))
            for a, b, c, d in exons:
                at += sum(len(number(v)) + 1 for v in (a, b, c, d))
                n = len(stretch(seqs[p], a, b))
                seen.add(((int(seq_at[p]) + a - 1) % 4 if n else 0, at % 4, n))
                at += n + 1
                n = len(stretch(genomic(), c, d))
                seen.add(((c - 1) % 4 if n else 0, at % 4, n))
                at += n + 1
    return seen


TAGS = (["digits_%d" % k for k in range(1, 11)] + ["zero", "negative", "int_min", "int_max", "flag_0", "flag_1", "flag_255"] +
        ["%s_%s" % (w, k) for w in ("est", "gen") for k in ("start_0", "start_negative", "start_at_len", "start_at_len_plus_1",
                                                            "start_at_len_plus_2", "end_before_start", "end_past_len", "first_byte",
                                                            "last_byte")] +
        ["group_of_8_bytes", "no_exons", "exons_1", "exons_63", "exons_64", "exons_65", "exons_128", "factorizations_2",
         "factorizations_3", "empty_header", "sequence_of_0", "sequence_of_1", "not_aligned_unaligned", "not_aligned_host"])


def tags_of(c, gl=GL):
    """what one case reaches"""
    t = set()
    if c["verdict"] != UL.U_ALIGNED:
        return {"not_aligned_unaligned" if c["verdict"] == UL.U_UNALIGNED else "not_aligned_host"}
    sl = len(c["seq"])
    if not c["facts"]:
        t.add("group_of_8_bytes")
    if len(c["facts"]) in (2, 3):
        t.add("factorizations_%d" % len(c["facts"]))
    if not c["header"]:
        t.add("empty_header")
    if sl in (0, 1):
        t.add("sequence_of_%d" % sl)
    for polya, polyad, exons in c["facts"]:
        for f in (polya, polyad):
            if f in (0, 1, 255):
                t.add("flag_%d" % f)
        if len(exons) in (0, 1, 63, 64, 65, 128):
            t.add("exons_%d" % len(exons) if exons else "no_exons")
        for e in exons:
            for v in e:
                t.add("zero" if v == 0 else "digits_%d" % len(str(abs(v))))
                if v < 0:
                    t.add("negative")
                if v in (INT_MIN, INT_MAX):
                    t.add("int_min" if v == INT_MIN else "int_max")
            for w, a, b, n in (("est", e[0], e[1], sl), ("gen", e[2], e[3], gl)):
                for k, hit in (("start_0", a == 0), ("start_negative", a < 0), ("start_at_len", a == n and n > 0),
                               ("start_at_len_plus_1", a == n + 1), ("start_at_len_plus_2", a == n + 2),
                               ("end_before_start", b < a and a >= 1), ("end_past_len", 1 <= a <= n < b),
                               ("first_byte", a == 1 and b >= 1 and n > 0), ("last_byte", 1 <= a <= n <= b)):
                    if hit:
                        t.add("%s_%s" % (w, k))
    return t


# ---- the program's own files ----------------------------------------------------------------------------------------
def original_genomic(gfa):
    """ef_seq.original_seq of genomic.txt: the lines behind the header, joined (ef_io.c: parse_records)"""
    lines = gfa.encode().split(b"\n")
    assert lines[0].startswith(b">")
    out = []
    for ln in lines[1:]:
        if ln.startswith(b">"):
            break
        out.append(ln.rstrip(b"\r\t \x0b\x0c"))
    return b"".join(out)


def est_headers(efa):
    """ef_seq.id of every entry of ests.txt, in input order"""
    return [ln[1:].rstrip(b"\r\t \x0b\x0c") for ln in efa.encode().split(b"\n") if ln.startswith(b">")]


def program_texts(exe, gfa, efa, retain, cwd, env=None):
    """(records, raw-multifasta-out.txt, processed-ests.txt) of one run of the binary `exe`"""
    rec = UL.program_records(exe, gfa, efa, retain, cwd, env)
    with open(os.path.join(cwd, "raw-multifasta-out.txt"), "rb") as f:
        raw = f.read()
    with open(os.path.join(cwd, "processed-ests.txt"), "rb") as f:
        pests = f.read()
    return rec, raw, pests


def entries(pests):
    """processed-ests.txt -> ([header], [sequence])"""
    lines = pests.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1 and all(h.startswith(b">") for h in lines[0:-1:2])
    return [h[1:] for h in lines[0:-1:2]], lines[1:-1:2]


def per_est(rec, raw, pests):
    """{est_index: (its lines of raw-multifasta-out.txt, its entry of processed-ests.txt)}: the files cut by the records'
    own counts (3 lines per factorization and one per exon; two per entry)"""
    raw_lines, pests_lines = raw.split(b"\n"), pests.split(b"\n")
    out, r, p = {}, 0, 0
    for _, _, est_index, facts in UL.read_blob(rec):
        n = sum(3 + len(f[2]) for f in facts)
        out[est_index] = (b"".join(ln + b"\n" for ln in raw_lines[r:r + n]), b"".join(ln + b"\n" for ln in pests_lines[p:p + 2]))
        r += n
        p += 2
    assert raw_lines[r:] == [b""] and pests_lines[p:] == [b""]
    return out
