"""The enumeration stage (pgpu_pairing_plan_run_candidate_lists / pgpu_index_candidate_lists, pintron_amd/csrc/pgpu_enum.hip)
restated in plain Python over cand_lib.update_embedding and cand_lib.parse, the host's ef_chain_candidates through
tests/hostcheck/libestfact_check.so, the fixture tests/golden/candidate_lists.json.gz and the hand-made records over
cand_lib.hand_sequence().  Shared by tests/test_enum_cpu.py, tests/test_gpu_enum.py, tools/make_enum_golden.py and
tools/enum_cost.py.

The restatement keeps an embedding as a list and recurses as the host does (get_subtree_embeddings,
src/est-factorizations.c:597-762); the kernel keeps a pool of linked records and an explicit stack.  The caps are checked
where include/pintron_gpu.h says: the embeddings behind every creation, the list behind every append."""
import ctypes as C
import gzip
import json
import os
import struct

import cand_lib as CL

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "candidate_lists.json.gz")

NONE, CYCLIC, RANGE, LISTS = range(4)
CAP_LIST, CAP_EMBEDDINGS = 1, 2
MAX_LIST, MAX_EMBEDDINGS = 64, 512

RELATION_TAGS = ("longer_2", "longer_1", "shorter_0", "shorter_1", "equal_0", "equal_2", "equal_1")
TAGS = ("flag_unavailable", "flag_too_complex") + RELATION_TAGS + (
    "removal_then_append", "stop_at_0", "diamond", "second_root", "leaf_not_sink", "root_without_candidate", "empty_graph",
    "one_path", "one_path_refused", "vertices_64", "degree_32", "cyclic", "cap_list", "cap_embeddings", "list_64",
    "embeddings_512", "no_vertex", "source_copy")
# tags a case can carry only once by construction (tests/test_enum_cpu.py asks three cases of every other tag)
ONCE = ("list_64", "embeddings_512", "no_vertex", "cap_embeddings")
# the rules a wrong implementation might have instead; the fixture notices each (tests/test_enum_cpu.py)
WRONG_RULES = ("no_pruning", "ignore_k0", "keep_removed", "reverse_roots", "visited_only_roots")


class Refused(Exception):
    def __init__(self, kind, detail):
        Exception.__init__(self)
        self.kind, self.detail = kind, detail


def inside(a, b):
    return not (a[0] < b[0] or a[0] + a[2] > b[0] + b[2]) and not (a[1] < b[1] or a[1] + a[2] > b[1] + b[2])


def relation(add, cmp, info=None):
    """maximality_relation (:1362-1460): 2 add is maximal, 1 both, 0 cmp is"""
    if len(add) > len(cmp):
        r, tag = (2 if all(inside(c, a) for a, c in zip(add, cmp)) else 1), "longer_"
    elif len(add) < len(cmp):
        r, tag = (0 if all(inside(a, c) for a, c in zip(add, cmp)) else 1), "shorter_"
    else:
        tag = "equal_"
        if all(inside(a, c) for a, c in zip(add, cmp)):
            r = 0
        else:
            r = 2 if all(inside(c, a) for a, c in zip(add, cmp)) else 1
    if info is not None:
        info[tag + str(r)] = True
    return r


def exons_of(emb, L):
    """get_factorizations_from_embeddings (:1292-1356) for one embedding"""
    exons = []
    for p, t, l in emb:
        if not exons or t - exons[-1][3] - 1 > 2 * L:
            exons.append([p, p + l - 1, t, t + l - 1])
        else:
            exons[-1][1], exons[-1][3] = p + l - 1, t + l - 1
    return [tuple(e) for e in exons]


def candidate_lists(rec, gen, L, min_intron, burset=CL.burset_adaptor, info=None, wrong=None):
    """One record -> (kind, detail, work, n_roots, [(root, n_pairs, exons)]).  `wrong`: one of WRONG_RULES, for the tests
    that show the fixture notices it."""
    info = {} if info is None else info
    flags, verts, adj = CL.parse(rec)
    if flags & CL.UNAVAILABLE:
        info["flag_unavailable"] = True
    if flags & CL.TOO_COMPLEX:
        info["flag_too_complex"] = True
    if flags & 3:
        return NONE, 0, 0, 0, []
    nv = len(verts)
    st = dict(work=0, created=0, peak=0)
    memo, visited, onstack = {}, set(), set()

    def create():
        st["created"] += 1
        if st["created"] > MAX_EMBEDDINGS:
            raise Refused(RANGE, CAP_EMBEDDINGS)

    def embeddings(v, as_root):
        if v in memo:
            info["diamond"] = True
            if wrong != "visited_only_roots":
                visited.add(v)
            return memo[v]
        if v in onstack:
            raise Refused(CYCLIC, 0)
        st["work"] += 1
        if wrong != "visited_only_roots" or as_root:
            visited.add(v)
        onstack.add(v)
        out = []
        if not adj[v]:
            create()
            out.append([list(verts[v])])
            if verts[v][0] != CL.SINK_P:
                info["leaf_not_sink"] = True
        for a in adj[v]:
            for e in embeddings(a, False):
                if verts[v][0] < 0 and e[0][0] != CL.SINK_P:
                    info["source_copy"] = True
                add = CL.update_embedding(e, verts[v], gen, L, min_intron, burset, info)
                if add is None:
                    continue
                st["work"] += 1
                create()
                if wrong == "no_pruning":
                    out.append(add)
                else:
                    rels, k0 = [], None                    # the host stops at the first 0: nothing behind it is compared
                    for k, c in enumerate(out):
                        rels.append(relation(add, c, info))
                        if rels[-1] == 0:
                            k0 = k
                            info["stop_at_0"] = True
                            break
                    front = range(len(out) if k0 is None else k0)
                    gone = {k for k in front if rels[k] == 2}
                    if gone and wrong != "keep_removed":
                        out[:] = [c for k, c in enumerate(out) if k not in gone]
                    if k0 is None or wrong == "ignore_k0":
                        if gone and k0 is None:
                            info["removal_then_append"] = True
                        out.append(add)
                st["peak"] = max(st["peak"], len(out))
                if len(out) > MAX_LIST:
                    raise Refused(RANGE, CAP_LIST)
        onstack.discard(v)
        memo[v] = out
        return out

    cands, n_roots = [], 0
    try:
        for r in (reversed(range(nv)) if wrong == "reverse_roots" else range(nv)):
            if r in visited:
                continue
            n_roots += 1
            embs = embeddings(r, True)
            if not embs:
                info["root_without_candidate"] = True
            if n_roots > 1 and embs and nv > 2:
                info["second_root"] = True
            for e in embs:
                cands.append((r, len(e), exons_of(e, L)))
    except Refused as x:
        info["cyclic" if x.kind == CYCLIC else ("cap_list" if x.detail == CAP_LIST else "cap_embeddings")] = True
        return x.kind, x.detail, 0, 0, []
    info["peak"], info["created"] = st["peak"], st["created"]
    if st["peak"] == MAX_LIST:
        info["list_64"] = True
    if st["created"] == MAX_EMBEDDINGS:
        info["embeddings_512"] = True
    if nv == 0:
        info["no_vertex"] = True
    if nv == 2 and not adj[0] and not adj[1]:
        info["empty_graph"] = True
    if nv == CL.MAX_VERTICES:
        info["vertices_64"] = True
    if any(len(a) >= 32 for a in adj):
        info["degree_32"] = True
    if CL.path_of(verts, adj) is not None:
        info["one_path" if cands else "one_path_refused"] = True
    return LISTS, 0, st["work"], n_roots, cands


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t))


# ---- the host's ef_chain_candidates -------------------------------------------------------------------------------
_host = {}


def host_candidate_lists(rec, gen_c, L, min_intron):
    """ef_chain_candidates (pintron_amd/host/ef_fact.c) on one record; the same tuple as candidate_lists().  Not for a record
    the restatement calls CYCLIC: the host does not return.  It has no cap either."""
    if not _host:
        H = CL.host_lib()
        H.ef_chain_candidates.restype = C.c_uint
        H.ef_chain_candidates.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t] + [C.POINTER(C.c_uint)] * 4
        ecap, ccap = 1 << 17, 1 << 14                          # the buffers are made once: tools/enum_cost.py times the calls
        _host.update(H=H, cfg=C.create_string_buffer(4096), ecap=ecap, ccap=ccap, ex=(C.c_int32 * (4 * ecap))(),
                     first=(C.c_uint * (ccap + 1))(), root=(C.c_uint * ccap)(), pairs=(C.c_uint * ccap)())
        H.ef_config_defaults(_host["cfg"])
    H, cfg, ex, first, root, pairs = (_host[k] for k in ("H", "cfg", "ex", "first", "root", "pairs"))
    struct.pack_into("<Ii", cfg, 0, L, min_intron)
    nc, ne, nr, work = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
    kind = H.ef_chain_candidates(rec, cfg, gen_c, ex, _host["ecap"], first, root, pairs, _host["ccap"], C.byref(nc), C.byref(ne),
                                 C.byref(nr), C.byref(work))
    if kind == 0:
        return NONE, 0, 0, 0, []
    assert nc.value <= _host["ccap"] and ne.value <= _host["ecap"]
    cands = [(root[c], pairs[c], [tuple(ex[4 * k:4 * k + 4]) for k in range(first[c], first[c + 1])]) for c in range(nc.value)]
    return LISTS, 0, work.value, nr.value, cands


# ---- hand-made records over cand_lib.hand_sequence() --------------------------------------------------------------
V = (100, 2000, 40)                 # the vertex the alternatives hang on
X = (140, 2200, 40)                 # an extension of V that keeps both lengths (cand_lib: `two`)
Y_IN_X = (140, 2200, 30)            # ... one that lies inside X
Y_APART = (145, 2300, 40)           # ... one that neither holds X nor lies in it
Z = (180, 2400, 40)                 # an extension of X


def graph(pairings, edges):
    """source, the pairings, sink; edges as (from, to) over 's', 'k' and the pairings' indices, kept in the order given"""
    verts = [CL.SOURCE] + list(pairings) + [CL.SINK]
    ix = lambda x: 0 if x == "s" else (len(verts) - 1 if x == "k" else x + 1)
    adj = [[] for _ in verts]
    for a, b in edges:
        adj[ix(a)].append(ix(b))
    return verts, adj


def alternatives(v, first, second):
    """v with two ways on, `first` folded before `second`; a way is a list of pairings, the last one joined to the sink.
    Record order is position order: the pairings by p; the edges of a vertex stay in the order made."""
    pairings, edges = [v], [("s", 0)]
    for way in (first, second):
        at = 0
        for p in way:
            if p not in pairings:
                pairings.append(p)
            k = pairings.index(p)
            if (at, k) not in edges:
                edges.append((at, k))
            at = k
        edges.append((at, "k"))
    order = sorted(range(len(pairings)), key=lambda k: (pairings[k][0], k))
    back = {k: j for j, k in enumerate(order)}
    fix = lambda x: x if x in ("s", "k") else back[x]
    return graph([pairings[k] for k in order], [(fix(a), fix(b)) for a, b in edges])


def layered(widths, ways=0, long_ways=0):
    """Layers of widths[a] alternatives each, every vertex of a layer joined to every vertex of the next: prod(widths) paths.
    The alternatives of a layer differ in t alone, by more than their length, so no embedding holds another and no pruning
    fires: the list at the source holds one embedding per path.  `ways`: extra single vertices between source and sink,
    `long_ways`: extra chains of two; each adds one embedding to the source's list."""
    pairings, idx = [], []
    for a, w in enumerate(widths):
        idx.append([])
        for b in range(w):
            idx[-1].append(len(pairings))
            pairings.append((100 + 40 * a, 200 + 300 * a + 50 * b, 40))
    edges = [("s", k) for k in idx[0]]
    for a in range(len(widths) - 1):
        edges += [(x, y) for x in idx[a] for y in idx[a + 1]]
    edges += [(k, "k") for k in idx[-1]]
    for j in range(long_ways):
        pairings += [(100, 3400 + 3 * j, 40), (140, 3600 + 3 * j, 40)]
        edges += [("s", len(pairings) - 2), (len(pairings) - 2, len(pairings) - 1), (len(pairings) - 1, "k")]
    for j in range(ways):
        pairings.append((100, 3500 + 45 * j, 40))
        edges += [("s", len(pairings) - 1), (len(pairings) - 1, "k")]
    return graph(pairings, edges)


def created_by(widths, ways=0, long_ways=0):
    """embeddings layered(...) creates: per vertex one for every path from it to the sink, the sink's own, and the source's
    copies; an extra way its vertex's and the source's copy, a long one three"""
    paths, total = 1, 1
    for w in reversed(widths):
        total += w * paths
        paths *= w
    return total + paths + 2 * ways + 3 * long_ways


# The cap edges, constructed (no search was needed).  The list: three layers of four give 4 * 4 * 4 = 64 at the source, one
# extra way 65.  The pool: eight single layers above layers of 4, 4 and 3 create 1 + (3 + 12 + 48) + 8 * 48 + 48 = 496, eight
# extra ways make it 512; seven and a long one 513.  The source's list stays at 56.
LIST_64, LIST_65, LIST_80 = ([4, 4, 4], 0, 0), ([4, 4, 4], 1, 0), ([4, 4, 5], 0, 0)
EMB_512, EMB_513 = ([1] * 8 + [4, 4, 3], 8, 0), ([1] * 8 + [4, 4, 3], 7, 1)
assert created_by(*EMB_512) == MAX_EMBEDDINGS and created_by(*EMB_513) == MAX_EMBEDDINGS + 1


def hand_cases(L=15):
    """[(name, record, min_factor_len, min_intron_length)]: what the real graphs do not reach, one builder per tag, three
    places of the sequence each where tests/test_enum_cpu.py asks for three cases"""
    out = []

    def add(name, verts, adj, Lx=L, intron=40, flags=0):
        out.append((name, CL.record(verts, adj, flags=flags), Lx, intron))

    for k in range(3):
        d = 3 * k
        sh = lambda p: (p[0], p[1] + d, p[2])
        v, x, z, y_in, y_apart = sh(V), sh(X), sh(Z), sh(Y_IN_X), sh(Y_APART)
        add("longer_2_%d" % k, *alternatives(v, [y_in], [x, z]))            # [v, y] then [v, x, z] holds it: removed, appended
        add("longer_1_%d" % k, *alternatives(v, [y_apart], [x, z]))
        add("shorter_0_%d" % k, *alternatives(v, [x, z], [y_in]))           # [v, y] lies in [v, x, z]: a stop
        add("shorter_1_%d" % k, *alternatives(v, [x, z], [y_apart]))
        add("equal_0_%d" % k, *alternatives(v, [x], [y_in]))
        add("equal_2_%d" % k, *alternatives(v, [y_in], [x]))                # a removal followed by an append
        add("equal_1_%d" % k, *alternatives(v, [x], [y_apart]))
        # a diamond: x is reached from v and from w; memoised, entered once, its work counted once
        add("diamond_%d" % k, *graph([v, (105, 2010 + d, 40), x], [("s", 0), ("s", 1), (0, 2), (1, 2), (2, "k")]))
        # a vertex the source does not reach: a second root with a candidate of its own
        add("second_root_%d" % k, *graph([v, x, (150, 3000 + d, 40)], [("s", 0), (0, 1), (1, "k"), (2, "k")]))
        add("leaf_not_sink_%d" % k, *graph([v, x], [("s", 0), (0, 1)]))
        # a root with no candidate: its only way on is refused (the pairings too close: cand_lib's deltas_small)
        add("root_without_candidate_%d" % k, *graph([(100, 2000 + d, 20), (105 + k, 2300, 20)], [(0, 1), (1, "k")]))
        add("empty_graph_%d" % k, [CL.SOURCE, CL.SINK], [[], []], Lx=L + k)
        add("one_path_%d" % k, *CL.chain([v, x, z]))
        add("one_path_refused_%d" % k, *CL.chain([(100, 2000 + d, 20), (105 + k, 2300, 20)]))
        out.append(("flag_unavailable_%d" % k, CL.bare(CL.UNAVAILABLE | (CL.TOO_COMPLEX if k == 2 else 0)), L, 40))
        add("flag_too_complex_%d" % k, *CL.chain([v, x]), flags=CL.TOO_COMPLEX)
        # 64 vertices: a path of 60 with a branch at its end
        sixty = [(20 * j, 50 * j + d, 20) for j in range(60)]
        add("vertices_64_%d" % k, *graph(sixty + [(1200, 3100 + d, 20), (1200, 3300 + d, 20)],
                                         [("s", 0)] + [(j, j + 1) for j in range(59)] + [(59, 60), (59, 61), (60, "k"), (61, "k")]))
        # out-degree 32: v with 32 ways on that differ in t
        ways = [(140, 2200 + 50 * j + d, 40) for j in range(32)]
        add("degree_32_%d" % k, *graph([v] + ways, [("s", 0)] + [(0, 1 + j) for j in range(32)] + [(1 + j, "k") for j in range(32)]))
    # the cyclic ones: cand_lib's `cycle`, a self-loop, and a cycle the source does not reach
    verts, _ = CL.chain([V, X])
    add("cycle", verts, [[1], [2], [1], []])
    add("self_loop", verts, [[1], [1, 2], [3], []])
    add("cycle_unreached", [CL.SOURCE, V, X, (150, 3000, 40), (190, 3200, 40), CL.SINK], [[1], [2], [5], [4], [3], []])
    add("no_vertex", [], [])
    add("one_vertex", [CL.SOURCE], [[]])
    add("sink_before_source", [CL.SINK, CL.SOURCE], [[], []])
    add("edge_into_a_leaf_source", [CL.SOURCE, V, CL.SOURCE, CL.SINK], [[1], [2, 3], [], []])
    add("list_64", *layered(*LIST_64))
    add("list_65", *layered(*LIST_65))
    add("list_80", *layered(*LIST_80))
    add("embeddings_512", *layered(*EMB_512))
    add("embeddings_513", *layered(*EMB_513))
    return out


# ---- the fixture --------------------------------------------------------------------------------------------------
_fixture = []


def load_fixture():
    """({sequence name: bytes}, [case]); a case: dict(seq, name, record, L, min_intron, kind, detail, work, n_roots, cands
    [(root, n_pairs, [exon])], tags).  The sequences are cand_lib's.  Shared: do not modify."""
    if not _fixture:
        import base64
        seqs, _ = CL.load_fixture()
        doc = json.loads(gzip.open(FIXTURE).read())
        cases = []
        for seq, name, rec, L, mi, kind, detail, work, n_roots, cands, tags in doc["cases"]:
            cases.append(dict(seq=seq, name=name, record=base64.b64decode(rec), L=L, min_intron=mi, kind=kind, detail=detail,
                              work=work, n_roots=n_roots, cands=[(r, n, [tuple(e) for e in ex]) for r, n, ex in cands], tags=tags))
        _fixture.append((seqs, cases, doc["counts"]))
    return _fixture[0]


def answer_of(c):
    return c["kind"], c["detail"], c["work"], c["n_roots"], c["cands"]


# ---- the device's arrays --------------------------------------------------------------------------------------------
def expect_arrays(answers):
    """[(kind, detail, work, n_roots, cands)] -> (results, candidate table, exons) as the entries write them"""
    import numpy as np
    import pintron_amd.capi as capi
    res = np.zeros(len(answers), dtype=np.dtype(capi.ENUM_RESULT_DTYPE))
    table, ex = [], []
    for i, (kind, detail, work, n_roots, cands) in enumerate(answers):
        res[i] = (kind, detail, work, len(table) if kind == LISTS and cands else 0, len(cands), n_roots)
        for root, n_pairs, exons in cands:
            table.append((len(ex), len(exons), n_pairs, root, 0))
            ex += exons
    return (res, np.array(table, dtype=np.dtype(capi.ENUM_CANDIDATE_DTYPE)).reshape(-1),
            np.array(ex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1))


def answers_of_arrays(res, table, exons):
    """the reverse, for messages and for comparing a slice of a batch"""
    out = []
    for r in res:
        cands = []
        for c in table[int(r["first_candidate"]):int(r["first_candidate"]) + int(r["n_candidates"])]:
            ex = exons[int(c["first_exon"]):int(c["first_exon"]) + int(c["n_exons"])]
            cands.append((int(c["root"]), int(c["n_pairs"]), [tuple(int(x) for x in e) for e in ex.tolist()]))
        out.append((int(r["kind"]), int(r["detail"]), int(r["work"]), int(r["n_roots"]), cands))
    return out
