"""The candidate stage (pgpu_pairing_plan_run_candidates / pgpu_index_candidates, pintron_amd/csrc/pgpu_cand.hip) restated in
plain Python, the records it takes, the host's ef_chain_candidate through tests/hostcheck/libestfact_check.so, the fixture
tests/golden/candidates.json.gz and the hand-made records for what no real graph reaches.  Shared by
tests/test_cand_cpu.py, tests/test_gpu_cand.py and tools/make_candidates_golden.py.

The restatement keeps the embedding as a list, as update_embedding (src/est-factorizations.c:765-917) does, and makes the
exons from it front to back (:1292-1356); the kernel never stores it and makes them back to front.  Python's integers do
not wrap: the entry's validator keeps every input inside what int arithmetic holds."""
import ctypes as C
import gzip
import json
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "candidates.json.gz")

SOURCE_P, SINK_P, MARK_LEN = -2 ** 31, 2 ** 31 - 1 - 200, 200
SOURCE, SINK = (SOURCE_P, SOURCE_P, MARK_LEN), (SINK_P, SINK_P, MARK_LEN)
NONE, NOT_PATH, REFUSED, ONE = range(4)
TOO_COMPLEX, UNAVAILABLE = 1, 2
MAX_VERTICES, MAX_FACTOR_LEN, MAX_P_END = 64, 1 << 24, 1 << 29

# what a case can reach; the fixture's cover counts them (tests/golden/candidates.md)
TAGS = ("flag_unavailable", "flag_too_complex", "not_path", "refuse_deltas", "refuse_lengths", "refuse_diagonal",
        "refuse_last", "refuse_sink_source", "split", "clamp_node", "clamp_head", "scan", "empty_range", "tie",
        "node_at_sequence_end", "head_at_sequence_start", "merged_pairing", "source_sink_only", "vertices_64")
# The two guards of the adaptor a scan cannot reach on a record the entry accepts.  A scan needs an overlap on the EST and
# an intron, so the split ran with gap_on_t = big_delta - ref_delta - 1 >= 0: small_delta < big_delta, and every cut lies
# in [node.p + L, head.p + head.l - L].  Then cut1 <= node.t + small_delta - L < node.t + big_delta - L <= length - L (the
# head ends inside the sequence), and cut2 >= node.p + L - head.p + head.t > node.t + L (big_delta > small_delta): neither
# the terminator nor cut2 < 2 is met.  The restatement notes them all the same; the tests assert they never appear.
NEVER = ("sequence_end", "cut2_below_2")
# ways of not being a path, by the hand-made record's name
NOT_PATH_WAYS = ("branch", "cycle", "vertex_left_out", "wrong_first", "wrong_last", "one_vertex")


# ---- records ------------------------------------------------------------------------------------------------------
def record(vertices, adj, flags=0, meg_text=b"", edges_text=b"", n_edges=None):
    """One MEG record (layout: include/pintron_gpu.h): vertices [(p, t, l)], adj [[targets]] per vertex."""
    nv = len(vertices)
    first, tgt = [0], []
    for a in adj:
        tgt += a
        first.append(len(tgt))
    ne = len(tgt) if n_edges is None else n_edges
    out = struct.pack("<4I", nv, ne, flags, 0)
    out += b"".join(struct.pack("<3i", *v) for v in vertices)
    out += struct.pack("<%dH" % (nv + 1), *first) + bytes(tgt)
    out += b"\0" * (-len(out) % 4)
    out += struct.pack("<2I", len(meg_text), len(edges_text)) + meg_text + edges_text
    return out + b"\0" * (-len(out) % 4)


def bare(flags):
    """the 16 bytes of a record the MEG stage could not build"""
    return struct.pack("<4I", 0, 0, flags, 0)


def graph_of_meg_text(meg):
    """meg_write's text ("(p,t,l)" lines, "#adj#", "i-j" lines) -> (vertices, adj)"""
    head, tail = meg.decode().split("#adj#\n")
    verts = [tuple(int(x) for x in ln.strip("()").split(",")) for ln in head.splitlines()]
    adj = [[] for _ in verts]
    for ln in tail.splitlines():
        a, b = ln.split("-")
        adj[int(a)].append(int(b))
    return verts, adj


def parse(rec):
    """(flags, vertices, adj) of a record; a flagged one has no graph as far as the stage reads"""
    nv, ne, flags, _ = struct.unpack_from("<4I", rec, 0)
    if flags & 3:
        return flags, [], []
    verts = [struct.unpack_from("<3i", rec, 16 + 12 * k) for k in range(nv)]
    first = struct.unpack_from("<%dH" % (nv + 1), rec, 16 + 12 * nv)
    base = 16 + 12 * nv + 2 * (nv + 1)
    return flags, verts, [list(rec[base + first[k]:base + first[k + 1]]) for k in range(nv)]


# ---- the restatement ----------------------------------------------------------------------------------------------
def burset_adaptor(gen, cut1, cut2):
    """getBursetFrequency_adaptor (src/refine-intron.c:362-374) on the sequence as a C string"""
    import refine_lib as RL
    if cut2 < 2:
        return 0
    d = gen[cut1:cut1 + 2] if cut1 < len(gen) else b""
    return RL.burset_frequency(d, gen[cut2 - 2:cut2])


def path_of(verts, adj):
    """the path test of chain_embedding: the vertices in path order, or None"""
    nv = len(verts)
    if nv < 2 or nv > MAX_VERTICES or verts[0][0] != SOURCE_P:
        return None
    seen, path, k = set(), [], 0
    while True:
        if k in seen:
            return None
        seen.add(k)
        path.append(k)
        if len(adj[k]) == 0:
            break
        if len(adj[k]) != 1:
            return None
        k = adj[k][0]
        if k >= nv:
            return None
    if len(path) != nv or verts[path[-1]][0] != SINK_P:
        return None
    return path


def update_embedding(emb, node, gen, L, min_intron, burset, info):
    """update_embedding (:765-917): the embedding (a list of [p, t, l], head first) extended by node, or None"""
    head = emb[0]
    if head[0] == SINK_P:
        if node[0] < 0:
            info["refuse_sink_source"] = True
            return None
        return [list(node)]
    if node[0] < 0:
        return [list(x) for x in emb]
    small = head[0] + head[2] - node[0]
    big = head[1] + head[2] - node[1]
    fl = 2 * L
    if not (small >= fl and big >= fl):
        info["refuse_deltas"] = True
        return None
    if not small - (node[2] + head[2]) <= fl:
        info["refuse_lengths"] = True
        return None
    if not small - big <= fl:
        info["refuse_diagonal"] = True
        return None
    if small >= node[2] + head[2] and big >= node[2] + head[2]:
        head_p, head_t, head_l, node_l = head[0], head[1], head[2], node[2]
    else:
        info["split"] = True
        ref = min(small, big)
        len_node = ref // 2                                   # ref >= 2L > 0 here: C's division and Python's agree
        len_head = ref - len_node
        if len_node > node[2]:
            info["clamp_node"] = True
            len_node = node[2]
            len_head = ref - len_node
        elif len_head > head[2]:
            info["clamp_head"] = True
            len_head = head[2]
            len_node = ref - len_head
        head_l = len_head
        head_p = head[0] + head[2] - head_l
        head_t = head[1] + head[2] - head_l
        node_l = len_node
    overlap_on_p = small < node[2] + head[2]
    gap_on_p = head_p - node[0] - node_l - 1
    gap_on_t = head_t - node[1] - node_l - 1
    intron_len = gap_on_t - max(gap_on_p, 0)
    intron_on_t = intron_len >= 0 and (min_intron == 0 or intron_len >= min_intron)
    if overlap_on_p and intron_on_t:
        info["scan"] = info.get("scan", 0) + 1
        if node[1] + node[2] == len(gen):
            info["node_at_sequence_end"] = True
        if head[1] == 0:
            info["head_at_sequence_start"] = True
        best_freq, best_cut = -1, 0
        lo = max(node[0] + L, head[0])
        hi = min(head[0] + head[2] - L, node[0] + node[2])
        if lo > hi:
            info["empty_range"] = True
        freqs = []
        for cut in range(lo, hi + 1):
            c1, c2 = cut - node[0] + node[1], cut - head[0] + head[1]
            if c1 + 1 >= len(gen):
                info["sequence_end"] = True
            if c2 < 2:
                info["cut2_below_2"] = True
            f = burset(gen, c1, c2)
            freqs.append(f)
            if f >= best_freq:
                best_freq, best_cut = f, cut
        info["widest"] = max(info.get("widest", 0), len(freqs))
        if freqs and freqs.count(best_freq) > 1:
            info["tie"] = True
        d = best_cut - head[0]
        head_l, head_p, head_t = head[2] - d, head[0] + d, head[1] + d
        node_l = node[2] - (node[0] + node[2] - best_cut)
    if not (gap_on_t <= fl or intron_on_t):
        info["refuse_last"] = True
        return None
    return [[node[0], node[1], node_l], [head_p, head_t, head_l]] + [list(x) for x in emb[1:]]


def candidate(rec, gen, L, min_intron, burset=burset_adaptor, info=None):
    """One record -> (kind, work, n_pairs, exons [(EST_start, EST_end, GEN_start, GEN_end)])"""
    info = {} if info is None else info
    flags, verts, adj = parse(rec)
    if flags & UNAVAILABLE:
        info["flag_unavailable"] = True
    if flags & TOO_COMPLEX:
        info["flag_too_complex"] = True
    if flags & 3:
        return NONE, 0, 0, []
    path = path_of(verts, adj)
    if path is None:
        info["not_path"] = True
        return NOT_PATH, 0, 0, []
    if len(verts) == 2:
        info["source_sink_only"] = True
    if len(verts) == MAX_VERTICES:
        info["vertices_64"] = True
    work = len(verts)
    emb = [list(verts[path[-1]])]
    for k in reversed(path[:-1]):
        emb = update_embedding(emb, verts[k], gen, L, min_intron, burset, info)
        if emb is None:
            return REFUSED, work, 0, []
        work += 1
    exons = []
    for p, t, l in emb:
        if not exons or t - exons[-1][3] - 1 > 2 * L:
            exons.append([p, p + l - 1, t, t + l - 1])
        else:
            info["merged_pairing"] = info.get("merged_pairing", 0) + 1
            exons[-1][1], exons[-1][3] = p + l - 1, t + l - 1
    return ONE, work, len(emb), [tuple(e) for e in exons]


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t))


# ---- the entry's rules on its input (pintron_amd/csrc/pgpu_cand.h), restated --------------------------------------
def record_einval(rec, glen):
    if len(rec) < 16:
        return True
    nv, ne, flags, _ = struct.unpack_from("<4I", rec, 0)
    if flags & 3:
        return False
    if nv > MAX_VERTICES:
        return True
    o_first = 16 + 12 * nv
    o_tgt = o_first + 2 * (nv + 1)
    if len(rec) < o_tgt or ne > len(rec) - o_tgt:
        return True
    for k in range(nv):
        p, t, l = struct.unpack_from("<3i", rec, 16 + 12 * k)
        if p in (SOURCE_P, SINK_P):
            if t != p or l != MARK_LEN:
                return True
            continue
        if p < 0 or l < 0 or t < 0 or p + l > MAX_P_END or t + l > glen:
            return True
    first = struct.unpack_from("<%dH" % (nv + 1), rec, o_first)
    if any(b < a for a, b in zip((0,) + first, first)) or first[-1] > ne:
        return True
    return any(x >= nv for x in rec[o_tgt:o_tgt + ne])


def einval(blob, rec_first, glen, L):
    """what pgpu_index_candidates refuses as a whole"""
    if L == 0 or L > MAX_FACTOR_LEN:
        return True
    for a, b in zip(rec_first, rec_first[1:]):
        a, b = int(a), int(b)
        if b < a or b > len(blob) or a % 4:
            return True
        if record_einval(blob[a:b], glen):
            return True
    return False


# ---- the host's ef_chain_candidate --------------------------------------------------------------------------------
_host = []


def host_lib():
    if not _host:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostcheck"), "libestfact_check.so"], check=True)
        H = C.CDLL(os.path.join(HERE, "hostcheck", "libestfact_check.so"))
        H.ef_config_defaults.argtypes = [C.c_void_p]
        H.ef_chain_candidate.restype = C.c_uint
        H.ef_chain_candidate.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t] + [C.POINTER(C.c_uint)] * 3
        _host.append(H)
    return _host[0]


def host_candidate(rec, gen_c, L, min_intron):
    """ef_chain_candidate (pintron_amd/host/ef_fact.c) on one record; gen_c: the sequence as a ctypes string buffer (its
    terminator behind it).  The same tuple as candidate()."""
    H = host_lib()
    cfg = C.create_string_buffer(4096)                        # an ef_config: unsigned min_factor_len, int min_intron_length, ...
    H.ef_config_defaults(cfg)
    struct.pack_into("<Ii", cfg, 0, L, min_intron)
    cap = 64
    ex = (C.c_int32 * (4 * cap))()
    ne, npairs, work = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    kind = H.ef_chain_candidate(rec, cfg, gen_c, ex, cap, C.byref(ne), C.byref(npairs), C.byref(work))
    assert ne.value <= cap
    return kind, work.value, npairs.value, [tuple(ex[4 * k:4 * k + 4]) for k in range(ne.value)]


# ---- the sequences and graphs real inputs give --------------------------------------------------------------------
def real_inputs():
    """{name: (genomic fasta, ests fasta)} of the fixture's real graphs"""
    import meg_lib as M
    g = os.path.join(HERE, "golden")
    src = M.sweep_sources()["c2"]
    return {"c2": src[:2],
            "ambn": (open(os.path.join(g, "ambn", "genomic.txt")).read(), open(os.path.join(g, "ambn", "ests.txt")).read()),
            "issue13": (gzip.open(os.path.join(g, "issue13", "genomic.txt.gz")).read().decode(),
                        gzip.open(os.path.join(g, "issue13", "ests.txt.gz")).read().decode())}


def fixture_sets():
    """the parameter sets of the fixture's real graphs: (name, pgpu_meg_params as meg_lib has them)"""
    import meg_lib as M
    return [("defaults", M.DEFAULTS), ("neither", M.NEITHER), ("intron0", M.params(min_intron_length=0)),
            ("intron200", M.params(min_intron_length=200))]


def host_records(gfa, efa, prm):
    """The first-attempt graphs of meg_lib (host MEG code over the pairing oracle) as records, with the genomic sequence
    as the index sees it: ([record], genomic).  A graph the device would have to give up is a record all the same."""
    import meg_lib as M
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    recs = []
    for e in exp:
        verts, adj = graph_of_meg_text(e["meg"])
        if len(verts) > MAX_VERTICES:
            recs.append(bare(UNAVAILABLE))
        else:
            recs.append(record(verts, adj, flags=TOO_COMPLEX if e["complex"] else 0))       # without the two texts
    return recs, genomic


# ---- hand-made records --------------------------------------------------------------------------------------------
HAND_LEN = 4000


def hand_sequence():
    """A seeded sequence of HAND_LEN bases with what the hand-made cases need written into it: a stretch of one letter
    (every cut has the same frequency), and GT / AG pairs at chosen places."""
    import random
    rng = random.Random(765)
    g = bytearray(rng.choice(b"ACGT") for _ in range(HAND_LEN))
    g[1000:1400] = b"C" * 400                                 # frequency of CC..CC at every cut: a tie across any range
    return bytes(g)


def chain(pairings):
    """source -> the pairings in order -> sink"""
    verts = [SOURCE] + list(pairings) + [SINK]
    return verts, [[k + 1] for k in range(len(verts) - 1)] + [[]]


def hand_cases(L=15):
    """[(name, record, min_factor_len, min_intron_length)] over hand_sequence(): what no real graph reaches, five of each
    where tests/test_cand_cpu.py asks for five."""
    n = HAND_LEN
    out = []

    def add(name, pairings, intron=40, Lx=L):
        out.append((name, record(*chain(pairings)), Lx, intron))

    # the first pairing of a chain is the node, the second the head it is folded onto
    for k in range(5):
        s = 10 * k
        # the first refusal: one of the deltas below 2L (the pairings too close on the EST, or on the sequence)
        add("deltas_small_%d" % k, [(100, 2000 + s, 20), (100 + 5 + k, 2300, 20)])
        add("deltas_big_%d" % k, [(100, 2000, 40), (160, 1980 - s, 40)])
        # the second: the EST gap between them longer than 2L
        add("lengths_%d" % k, [(100, 2000, 20), (151 + s, 2300, 20)])
        # the third: the EST runs ahead of the sequence by more than 2L
        add("diagonal_%d" % k, [(100, 2000, 30), (150 + k, 2000 + k, 30)])
        # an empty cut range: a node shorter than L, so node.p + L lies behind node.p + node.l; best_cut stays 0
        add("empty_range_%d" % k, [(100, 2000 + s, 10), (105, 2500 + s, 30)])
        # equal frequencies across a range: both sides of every cut lie in the stretch of one letter
        add("tie_%d" % k, [(100, 1010 + s, 40), (120 + k, 1200 + s, 40)])
    add("empty_range_then_a_node", [(60, 1500, 30), (100, 2000, 10), (105, 2500, 30)])
    add("last_refusal", [(100, 2000, 40), (145, 2080, 40)], intron=60)       # a genomic gap of 2L + 5 that is no intron
    add("last_accepts_gap_2L", [(100, 2000, 40), (145, 2070, 40)], intron=60)
    # a node whose occurrence ends on the sequence's last byte, and a head that begins on its first: the nearest a scan
    # comes to either end (see NEVER below)
    add("node_at_sequence_end", [(100, n - 40, 40), (110, n - 25, 25)], intron=0)
    add("head_at_sequence_start", [(120, 5, 40), (100, 0, 80)], intron=0)
    # the two clamps of the split
    add("clamp_node", [(100, 2000, 4), (102, 2002, 60)], intron=0)
    add("clamp_node_scan", [(100, 2000, 4), (102, 2102, 60)])
    add("clamp_head", [(100, 2000, 60), (150, 2050, 4)], intron=0)
    add("split_even", [(100, 2000, 40), (130, 2030, 40)])
    add("split_odd", [(100, 2000, 40), (131, 2031, 40)])
    out.append(("source_sink_only", record(*chain([])), L, 40))
    sixty_two = [(20 * k, 50 * k, 20) for k in range(62)]
    out.append(("vertices_64", record(*chain(sixty_two)), L, 40))
    out.append(("vertices_64_introns", record(*chain([(20 * k, 60 * k, 20) for k in range(62)])), L, 40))
    out.append(("vertices_64_backwards", record(*backwards(sixty_two)), L, 40))
    # each way of not being a path
    two = [(100, 2000, 40), (140, 2200, 40)]
    v, a = chain(two)
    out.append(("branch", record(v, [[1, 2], [2], [3], []]), L, 40))
    out.append(("cycle", record(v, [[1], [2], [1], []]), L, 40))
    out.append(("vertex_left_out", record(v, [[2], [2], [3], []]), L, 40))
    out.append(("wrong_first", record([two[0]] + v[1:], a), L, 40))
    out.append(("wrong_last", record(v[:-1] + [two[1]], a), L, 40))
    out.append(("sink_in_the_middle", record([SOURCE, two[0], SINK, two[1]], [[1], [3], [], [2]]), L, 40))
    out.append(("one_vertex", record([SOURCE], [[]]), L, 40))
    out.append(("no_vertex", record([], []), L, 40))
    out.append(("path_out_of_order", record([SOURCE, two[1], two[0], SINK], [[2], [3], [1], []]), L, 40))
    out.append(("flag_unavailable", bare(UNAVAILABLE), L, 40))
    out.append(("flag_too_complex", record(v, a, flags=TOO_COMPLEX), L, 40))
    out.append(("flag_both", bare(UNAVAILABLE | TOO_COMPLEX), L, 40))
    out.append(("second_source", record([SOURCE, two[0], SOURCE, two[1], SINK], [[1], [2], [3], [4], []]), L, 40))
    out.append(("second_sink", record([SOURCE, two[0], SINK, SINK], [[1], [2], [3], []]), L, 40))
    out.append(("other_L", record(*chain([(100, 2000, 40), (130, 2330, 40)])), 8, 0))
    return out


def backwards(pairings):
    """the same path with its pairings numbered against the path: vertex k + 1 is pairing n - 1 - k"""
    n = len(pairings)
    verts = [SOURCE] + list(reversed(pairings)) + [SINK]
    adj = [[n]] + [[n + 1]] + [[k] for k in range(1, n)] + [[]]
    # vertex 1 is the LAST pairing -> sink; vertex k + 1 -> vertex k; the source -> vertex n (the first pairing)
    return verts, adj


# ---- the fixture --------------------------------------------------------------------------------------------------
_fixture = []


def load_fixture():
    """({sequence name: bytes}, [case]); a case: dict(seq, name, record (bytes), L, min_intron, kind, work, n_pairs, exons,
    tags).  The real sequences are made from the inputs in the tree and checked against the digest the file holds.  Shared:
    do not modify."""
    if not _fixture:
        import base64
        import hashlib
        doc = json.loads(gzip.open(FIXTURE).read())
        seqs = {"hand": hand_sequence()}
        inputs = real_inputs()
        import meg_lib as M
        for name in doc["sequences"]:
            if name != "hand":
                seqs[name] = M.first_attempt_megs(*inputs[name])[1]
            assert hashlib.sha1(seqs[name]).hexdigest() == doc["sequences"][name]["sha1"], name
        cases = []
        for seq, name, rec, L, mi, kind, work, n_pairs, exons, tags in doc["cases"]:
            cases.append(dict(seq=seq, name=name, record=base64.b64decode(rec), L=L, min_intron=mi, kind=kind, work=work,
                              n_pairs=n_pairs, exons=[tuple(e) for e in exons], tags=tags))
        _fixture.append((seqs, cases))
    return _fixture[0]


def cover(cases):
    """{tag: cases}, {kind: cases}, scans, widest scan -- what tests/golden/candidates.md lists"""
    c = {"cases": len(cases), "kinds": [0, 0, 0, 0], "tags": {t: 0 for t in TAGS}}
    for x in cases:
        c["kinds"][x["kind"]] += 1
        for t in x["tags"]:
            c["tags"][t] += 1
    return c


# ---- batches for the device ---------------------------------------------------------------------------------------
def batch(records):
    """(blob, rec_first as numpy uint64) of a list of records"""
    import numpy as np
    first = np.zeros(len(records) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in records], out=first[1:])
    return b"".join(records), first


def expect_arrays(answers):
    """[(kind, work, n_pairs, exons)] -> (results, exons) as the entry writes them: the exons compact, in record order"""
    import numpy as np
    import pintron_amd.capi as capi
    res = np.zeros(len(answers), dtype=np.dtype(capi.CAND_RESULT_DTYPE))
    ex = []
    for i, (kind, work, n_pairs, exons) in enumerate(answers):
        res[i] = (kind, work, len(ex) if kind == ONE else 0, len(exons), n_pairs)
        ex += exons
    return res, np.array(ex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1)


def assert_layout(cname, struct_, dtype):
    """binding_lib.assert_layout for a struct with 16-bit fields"""
    import numpy as np
    import binding_lib as B
    size_of = dict(B.SIZE_OF, uint16_t=2)
    fields, size = B.header_struct(cname)
    assert [f for f, _ in fields] == [f for f, _ in struct_._fields_] == [f for f, _ in dtype], cname
    off, dt = 0, np.dtype(dtype)
    for f, ctype in fields:
        assert getattr(struct_, f).offset == off == dt.fields[f][1], (cname, f)
        assert getattr(struct_, f).size == size_of[ctype] == dt.fields[f][0].itemsize, (cname, f)
        off += size_of[ctype]
    assert off == size == C.sizeof(struct_) == dt.itemsize, cname
