"""The device MEG stage (pgpu_pairing_plan_run_meg, pintron_amd/csrc/pgpu_meg.hip) against the host MEG code over
the pairing oracle (tests/hostcheck/meg_check, first-attempt mode): the expectation, the rule that says when the
device must give up, the parameter sets and the crafted inputs aimed at the kernel's caps.  Shared by
tests/test_meg_cases_cpu.py (proves on the CPU that every input reaches its target), tests/test_gpu_meg.py and
tests/test_gpu_pairings.py.

The availability rule.  The kernel builds a graph in fixed arrays: PGPU_MEG_MAX_VERTICES = 64 vertices ever created
(source, sink, pairings, the vertices the compaction makes), PGPU_MEG_MAX_DEGREE = 32 entries per adjacency or
incidence list, 1024 DFS stack entries.  From the `@@stats` line of meg_check a record
  * MUST be unavailable when pairings + 2 + created > 64, or a list is longer than 32 after build_edge_set (lists
    only shrink in the simplification and the reduction) or at any moment of the compaction;
  * MUST be available otherwise, provided the DFS cannot overflow: the reduction is off, or 2 x vertices + edges
    after the simplification <= 1024 (every push is a root, a re-push of the vertex being opened, or one edge);
  * is GREY in the remaining case only (within the caps, stack bound not shown): either answer, but counted.
An available record is compared byte for byte."""
import hashlib
import os
import random
import subprocess
import tempfile
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_VERTICES, MAX_DEGREE, MAX_STACK = 64, 32, 1024          # include/pintron_gpu.h, pgpu_meg.hip

Counts = namedtuple("Counts", "v e adj inc")

# ---- parameter sets -----------------------------------------------------------------------------------------------
DEFAULTS = dict(min_factor_len=15, min_intron_length=40, max_intron_length=0, max_pairings_in_MEG=80,
                max_prefix_discarded_rate=0.6, max_suffix_discarded_rate=0.6, max_freq_shortest_pairing=0.4,
                trans_red=True, short_edge_comp=True)
_OPTION = dict(min_factor_len="--min-factor-length", min_intron_length="--min-intron-length",
               max_intron_length="--max-intron-length", max_pairings_in_MEG="--max-pairings-in-CMEG",
               max_prefix_discarded_rate="--max-prefix-discarded-rate", max_suffix_discarded_rate="--max-suffix-discarded-rate",
               max_freq_shortest_pairing="--max-shortest-pairing-frequence")


def params(**kw):
    """A complete pgpu_meg_params as the keyword arguments of capi.PairingPlan.run_meg."""
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def argv_of(prm):
    """The same parameters as est-fact's command line (what meg_check takes)."""
    out = []
    for k, opt in _OPTION.items():
        if prm[k] != DEFAULTS[k]:
            out.append("%s=%r" % (opt, prm[k]))
    if not prm["trans_red"]:
        out.append("--no-transitive-reduction")
    if not prm["short_edge_comp"]:
        out.append("--no-short-edge-compaction")
    return out


NEITHER = params(trans_red=False, short_edge_comp=False)


def shortest_intron(exons):
    return min(b[0] - a[1] for a, b in zip(exons, exons[1:]))


def sweep_sets(exons):
    """The parameter sets of the sweep, [(name, params)]: every field of pgpu_meg_params off its default in at least
    one.  `exons` is the gene model of the sample; the one value that depends on it is computed here."""
    return [
        ("L12", params(min_factor_len=12)),
        ("L18", params(min_factor_len=18)),
        ("L20-intron60", params(min_factor_len=20, min_intron_length=60)),
        ("intron0", params(min_intron_length=0)),
        ("intron25", params(min_intron_length=25)),
        ("intron60", params(min_intron_length=60)),
        ("maxintron3000", params(max_intron_length=3000)),
        ("maxintron-below-shortest", params(max_intron_length=shortest_intron(exons) // 2)),
        ("cmeg6", params(max_pairings_in_MEG=6, max_freq_shortest_pairing=0.1)),
        ("cmeg0", params(max_pairings_in_MEG=0)),
        ("cmeg0-freq0.1", params(max_pairings_in_MEG=0, max_freq_shortest_pairing=0.1)),      # 0 = no limit, not "every graph is over it"
        ("discarded-0.2-0.3", params(max_prefix_discarded_rate=0.2, max_suffix_discarded_rate=0.3)),
        ("discarded-0-1", params(max_prefix_discarded_rate=0.0, max_suffix_discarded_rate=1.0)),
        ("no-reduction", params(trans_red=False)),
        ("no-compaction", params(short_edge_comp=False)),
        ("neither", NEITHER),
    ]


# ---- the expectation ----------------------------------------------------------------------------------------------
_cache = {}
_built = []


def meg_check_binary():
    if not _built:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostcheck"), "meg_check"], check=True)
        _built.append(os.path.join(HERE, "hostcheck", "meg_check"))
    return _built[0]


def parse_stats(line):
    assert line.startswith("@@stats "), line
    st = {}
    for item in line.split()[1:]:
        k, v = item.split("=")
        st[k] = Counts(*map(int, v.split(","))) if "," in v else (v if k == "clause" else int(v))
    assert set(st) == {"pairings", "build", "simp", "red", "end", "created", "peak", "clause"}, line
    return st


def parse_first_attempt(text):
    out = []
    for blk in text.split("@@end\n")[:-1]:
        head, cx, stats, rest = blk.split("\n", 3)
        meg, edges = rest.split("@@edges\n")
        out.append(dict(seq=head[len("@@seq "):].encode(), complex=int(cx.split()[1]), stats=parse_stats(stats),
                        meg=meg.encode(), edges=edges.encode()))
    return out


def first_attempt_megs(genomic_fasta, ests_fasta, prm=DEFAULTS):
    """Host MEG code (pinned against the reference's megs.txt in test_host_meg.py and test_options_pin.py) over the
    pairing oracle: the first-attempt graph of every prepared sequence under `prm`, and the genomic sequence as the
    index sees it.  One meg_check run per (input, parameters) and process; the result is shared, do not modify it."""
    key = (hashlib.sha1((genomic_fasta + "\0" + ests_fasta).encode()).hexdigest(), tuple(argv_of(prm)))
    if key not in _cache:
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "genomic.txt"), "w") as f:
                f.write(genomic_fasta)
            with open(os.path.join(d, "ests.txt"), "w") as f:
                f.write(ests_fasta)
            subprocess.run([meg_check_binary()] + argv_of(prm), cwd=d, check=True,
                           env=dict(os.environ, MEG_CHECK_FIRST_ATTEMPT="1"), stderr=subprocess.DEVNULL)
            recs = parse_first_attempt(open(os.path.join(d, "megs-first.txt")).read()) if os.path.exists(os.path.join(d, "megs-first.txt")) else []
            _cache[key] = (recs, open(os.path.join(d, "genomic-prepared.txt"), "rb").read())
    return _cache[key]


def availability(stats, prm):
    """'unavailable', 'available' or 'grey' (module docstring)."""
    if (stats["pairings"] + 2 + stats["created"] > MAX_VERTICES or max(stats["build"].adj, stats["build"].inc) > MAX_DEGREE
            or stats["peak"] > MAX_DEGREE):
        return "unavailable"
    if not prm["trans_red"] or 2 * stats["simp"].v + stats["simp"].e <= MAX_STACK:
        return "available"
    return "grey"


def expected_size(e, prm):
    """Bytes of the device record of an expectation (layout: include/pintron_gpu.h); 16 for one that must be unavailable."""
    if availability(e["stats"], prm) == "unavailable":
        return 16
    nv, ne = e["stats"]["end"].v, e["stats"]["end"].e
    graph = (16 + 12 * nv + 2 * (nv + 1) + ne + 3) & ~3
    return (graph + 8 + len(e["meg"]) + len(e["edges"]) + 3) & ~3


def check_records(exp, recs, prm, what=""):
    """Device records (capi.parse_meg_record) against the expectation: the flag follows the rule, an available record
    is exact -- verdict, both texts, and the structured part says what the text says.  Returns the number of grey records."""
    assert len(exp) == len(recs), (what, len(exp), len(recs))
    n_grey = 0
    for k, (e, r) in enumerate(zip(exp, recs)):
        rule = availability(e["stats"], prm)
        where = (what, k, rule, e["stats"])
        if rule == "grey":
            n_grey += 1
        assert r["flags"] & ~3 == 0, where
        if r["flags"] & 2:
            assert rule != "available", where
            assert r["flags"] == 2 and r["n_vertices"] == 0 and r["n_edges"] == 0 and r["size"] == 16, where
            continue
        assert rule != "unavailable", where
        assert (r["flags"] & 1) == e["complex"], where
        assert r["meg_text"] == e["meg"], where
        assert r["edges_text"] == e["edges"], where
        lines = e["meg"].decode().split("#adj#\n")
        verts = [tuple(int(x) for x in ln.strip("()").split(",")) for ln in lines[0].splitlines()]
        assert [tuple(v) for v in r["vertices"]] == verts, where
        edges = [tuple(int(x) for x in ln.split("-")) for ln in lines[1].splitlines()]
        assert [(a, t) for a, adj in enumerate(r["adj"]) for t in adj] == edges, where
        assert r["n_vertices"] == len(verts) == e["stats"]["end"].v and r["n_edges"] == len(edges) == e["stats"]["end"].e, where
        assert r["size"] == r["used"] == expected_size(e, prm), where
    return n_grey


def parse_record(rec):
    """capi.parse_meg_record plus the header counts and the sizes (bytes received, bytes the layout accounts for)."""
    import struct
    import pintron_amd.capi as capi
    r = capi.parse_meg_record(rec)
    r["n_vertices"], r["n_edges"] = struct.unpack_from("<2I", rec, 0)
    r["size"] = len(rec)
    if not r["flags"] & 2:
        graph = (16 + 12 * r["n_vertices"] + 2 * (r["n_vertices"] + 1) + r["n_edges"] + 3) & ~3
        end = graph + 8 + len(r["meg_text"]) + len(r["edges_text"])
        r["used"] = (end + 3) & ~3
        assert rec[end:r["used"]] == b"\0" * (r["used"] - end)            # the padding is part of the record
    return r


def device_records(ctx, genomic, seqs, prm, rate=0.2, resident=False):
    """A fresh index and plan: pairings at prm's min_factor_len, then the MEG stage."""
    import pintron_amd.capi as capi
    idx = capi.Index(ctx, genomic)
    plan = capi.PairingPlan(ctx, idx, seqs, resident=resident)
    try:
        plan.run(prm["min_factor_len"], rate)
        plan.run_meg(**prm)
        return [parse_record(r) for r in plan.fetch_meg()]
    finally:
        plan.close()
        idx.close()


# ---- workload sources ---------------------------------------------------------------------------------------------
def _with_short_gaps(gfa, efa):
    """The source plus three ESTs that skip 36, 45 and 55 genomic bases: gaps between 2 L + 3 and the minimum intron
    length, the only ones remove_useless_edges looks at (the gene's own introns are 500 bases and more)."""
    g = gfa.split("\n")[1]
    for k, d in enumerate((36, 45, 55)):
        a = 1000 + 700 * k
        efa += ">/gb=GAP%05d /clone_end=3'\n%s\n" % (k, g[a:a + 120] + g[a + 120 + d:a + 240 + d])
    # ... and one with 85 pairings of 20 bases each (pieces 500 bases apart in the genomic sequence, one foreign base
    # between them): the only graph with more than the default max_pairings_in_MEG = 80 vertices, so the only one the
    # CMEG clause decides under the defaults -- on the host; the device has to give it up
    est = ""
    for k in range(85):
        a, b = 2000 + 500 * k, 2000 + 500 * (k + 1)
        est += g[a:a + 20] + next(c for c in "ACGT" if c != g[a + 20] and c != g[b - 1])
    efa += ">/gb=GAP%05d /clone_end=3' /fixed_strand=1\n%s\n" % (3, est)
    return gfa, efa


def sweep_sources():
    """{name: (genomic fasta, ests fasta, exons of the gene model)}: a C2-shaped sample (50 kb, 150 ESTs, both
    strands) and the region-start repeats, each with the three short-gap ESTs."""
    from pintron_amd import synth
    w = synth.make("C2", n_est=150, seed=23)
    return {"c2": _with_short_gaps(w.genomic_fasta(), w.ests_fasta()) + (w.exons,),
            "repeats": _with_short_gaps(*synth.make_region_start_repeats()) + (synth.make("C2", n_est=10).exons,)}


# ---- crafted inputs -----------------------------------------------------------------------------------------------
# One 60 kb genomic sequence.  Its first 6 kb stay as drawn and give the ordinary ESTs; behind them one slot every
# 150 bases takes a planted piece.  A UNIT is a 20-base word planted k times, every copy between two 'C's, and
# written into an EST between two 'A's: the occurrences are left-maximal and end with the unit, so the EST gets
# exactly k pairings (p, t_1..t_k, 20) at the unit's position.  Units further than 2 L + 1 apart in the EST have no
# edge between them; a vertex in the first 60 % of the EST without a predecessor hangs off the source, one that ends
# in the last 40 % without a successor goes to the sink.
SLOT0, SLOT = 6200, 150
CAP_INTRON = 100          # max_intron_length of the `tp50` case: a unit reaches its partner 6 bases on, not the next slot


class _Crafter:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.g = bytearray(self.rng.choice(b"ACGT") for _ in range(60000))
        self.next_slot = 0
        self.ests = []              # (label, sequence)

    def rs(self, n, al=b"CGT"):
        return bytes(self.rng.choice(al) for _ in range(n))

    def unit(self):
        return b"G" + self.rs(18, b"ACGT") + b"T"

    def plant(self, piece):
        at = SLOT0 + SLOT * self.next_slot
        assert len(piece) < SLOT - 20 and at + len(piece) < len(self.g) - 200
        self.g[at:at + len(piece)] = piece
        self.next_slot += 1
        return at

    def copies(self, unit, k):
        for _ in range(k):
            self.plant(b"C" + unit + b"C")

    def est(self, label, seq):
        self.ests.append((label, bytes(seq)))

    def ordinary(self, label, at, n=300, subs=()):
        e = bytearray(self.g[at:at + n])
        for s in subs:
            e[s] = b"ACGT"[(b"ACGT".index(e[s]) + 1) % 4]
        self.est(label, e)


def in_est(unit):
    return b"A" + unit + b"A"


def crafted():
    """(genomic fasta, ests fasta, labels): the inputs aimed at the caps, each over-cap pattern between two ordinary
    ones.  What every label is for: TARGETS below and tests/test_meg_cases_cpu.py."""
    c = _Crafter(20260)
    # pairings 61, 62, 63: four units of 15 copies, interleaved in the genomic sequence so that copy i of a unit
    # reaches the copies j >= i of the next one (degrees up to 15, ~400 edges: te > 5 tp), then a unit of 1, 2 or 3
    four = [c.unit() for _ in range(4)]
    for _ in range(15):
        for u in four:
            c.copies(u, 1)
    tails = {}
    for k in (1, 2, 3):
        tails[k] = c.unit()
        c.copies(tails[k], k)
    body = c.rs(20) + b"".join(in_est(u) + c.rs(4) for u in four)
    # lists of 32 and 33: a unit in the first 40 % (source's out-list), in the last 40 % (sink's in-list), and in
    # front of a unit with one copy behind all of them (that copy's in-list and the source's out-list)
    u32, u33 = c.unit(), c.unit()
    c.copies(u32, 32)
    behind32 = c.unit()
    c.copies(behind32, 1)
    c.copies(u33, 33)
    behind33 = c.unit()
    c.copies(behind33, 1)
    lone = [c.unit() for _ in range(4)]
    for u in lone:
        c.copies(u, 1)
    # tp >= 50 inside the caps: 26 x (unit, 4 bases, partner); with max_intron_length = CAP_INTRON every unit reaches
    # its own partner only: source -> 26 -> 26 -> sink
    ua, ub = c.unit(), c.unit()
    for _ in range(26):
        c.plant(b"C" + ua + b"C" + c.rs(4) + b"C" + ub + b"C")

    k = [0]

    def ordinary(subs=()):
        c.ordinary("ordinary", 300 + 330 * k[0], subs=subs)
        k[0] += 1

    ordinary()
    for n in (1, 2, 3):
        c.est("pairings%d" % (60 + n), body + in_est(tails[n]) + c.rs(20))
        ordinary(subs=(100,) if n == 2 else ())
    for n, u, b in ((32, u32, behind32), (33, u33, behind33)):
        c.est("out%d" % n, c.rs(6) + in_est(u) + c.rs(120) + in_est(lone[0]) + c.rs(30))
        ordinary()
        c.est("in%d" % n, c.rs(30) + in_est(lone[1]) + c.rs(120) + in_est(u) + c.rs(6))
        ordinary()
        c.est("both%d" % n, c.rs(40) + in_est(u) + c.rs(5) + in_est(b) + c.rs(40))
        ordinary()
        c.est("density%d" % n, c.rs(89) + in_est(u) + c.rs(89))        # 200 bases: tp = n + 2 > 2 * 200 / 15
        ordinary()
    c.est("tp50", c.rs(229) + in_est(ua) + c.rs(3) + in_est(ub) + c.rs(221))
    ordinary()
    # compaction: a substitution every 20 bases cuts a 620-base match into 31 pairings on one diagonal, one base
    # apart; the compaction joins them pairwise, pass after pass, and creates far more than 64 - 33 vertices
    c.ordinary("compaction-over", 450, n=620, subs=range(19, 620, 20))
    ordinary()
    # ... and at a size that fits: vertices made, and made vertices removed again
    c.ordinary("compaction-4", 1500, n=300, subs=(60, 120, 180, 240))
    c.ordinary("compaction-9", 2500, n=300, subs=range(29, 300, 30))
    ordinary()
    assert 300 + 330 * k[0] < SLOT0
    gfa = ">chrK:1:%d:+1\n%s\n" % (len(c.g), c.g.decode())
    efa = "".join(">/gb=CAP%05d /clone_end=3' /fixed_strand=1\n%s\n" % (i, s.decode()) for i, (_, s) in enumerate(c.ests))
    return gfa, efa, [label for label, _ in c.ests]


CAPS_INTRON = params(max_intron_length=CAP_INTRON)
NO_COMPACTION = params(short_edge_comp=False)
# the parameter sets the crafted input is run under
CRAFTED_SETS = [("defaults", DEFAULTS), ("neither", NEITHER), ("maxintron%d" % CAP_INTRON, CAPS_INTRON), ("no-compaction", NO_COMPACTION)]


# ---- degenerate patterns ------------------------------------------------------------------------------------------
def degenerate(n_total, L=15):
    """(genomic fasta, ests fasta) with n_total prepared sequences: patterns of L - 1, L and L + 1 bases, one without
    any pairing, one of Ns only, between ordinary ones (fixed strand: one prepared sequence per entry)."""
    rng = random.Random(77)
    g = bytes(rng.choice(b"ACGT") for _ in range(8000))
    special = [g[500:500 + L - 1], g[700:700 + L], g[900:900 + L + 1], bytes(rng.choice(b"ACGT") for _ in range(120)), b"N" * 60]
    ests = []
    for k in range(n_total):
        if k % 2 == 1 and k // 2 < len(special):
            ests.append(special[k // 2])
        else:
            at = 1000 + 97 * k
            e = bytearray(g[at:at + 200])
            if k % 3 == 0:
                e[100] = b"ACGT"[(b"ACGT".index(e[100]) + 1) % 4]
            ests.append(bytes(e))
    if n_total == 65:                        # the 65th pattern, alone in the kernel's second block, is a special one
        ests[64] = special[1]
    gfa = ">chrD:1:%d:+1\n%s\n" % (len(g), g.decode())
    efa = "".join(">/gb=DEG%05d /clone_end=3' /fixed_strand=1\n%s\n" % (i, s.decode()) for i, s in enumerate(ests))
    return gfa, efa


def rerun_input():
    """(genomic fasta, ests fasta) for the reruns on one plan: 60 ESTs with a substitution every 16..35 bases.  The
    compaction folds each of them into one vertex, so with both simplifications off the records are several times
    larger; the matches of 15 bases disappear at min_factor_len 16."""
    rng = random.Random(99)
    g = bytes(rng.choice(b"ACGT") for _ in range(24000))
    ests = []
    for k in range(60):
        e = bytearray(g[300 + 350 * k:600 + 350 * k])
        for s in range(15 + k % 20, 300, 16 + k % 20):
            e[s] = b"ACGT"[(b"ACGT".index(e[s]) + 1) % 4]
        ests.append(bytes(e))
    gfa = ">chrR:1:%d:+1\n%s\n" % (len(g), g.decode())
    efa = "".join(">/gb=RER%05d /clone_end=3' /fixed_strand=1\n%s\n" % (i, s.decode()) for i, s in enumerate(ests))
    return gfa, efa
