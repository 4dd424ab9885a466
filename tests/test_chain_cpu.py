"""CPU: the restatement of pgpu_index_refine_chains (tests/chain_lib.py) against what the reference's refinement loop left
(tests/golden/refine_chains.json.gz), the cover of that fixture, and the binding's layout against the header."""
import ctypes as C
import os
import re

import numpy as np

import binding_lib as BL
import chain_lib as CL
import refine_lib as RL

HEADER = BL.HEADER


def test_restatement_equals_the_fixture_on_every_chain():
    gen, chains = CL.load_fixture()
    for k, c in enumerate(chains):
        got = CL.chain(c["est"], gen, c["exons"], c["settings"])
        assert got == (CL.OK, c["done"], c["dropped_first"], c["exons_after"], c["steps"]), (k, got, c)
        assert c["done"] == len(c["exons"]) - 1 and c["steps"][0] == 0


def test_the_fixture_covers_what_it_must():
    """The ten paths at a chain's first intron and at a later one -- but `attached-first` (path 0) is the branch of
    first_intron (:127-135) and `attached-later` (path 1) the one without it (:136-140), and the loop sets first_intron
    for the chain's first intron alone: each of the two can be met at one kind of place only, so nine paths are asked
    for at either place."""
    gen, chains = CL.load_fixture()
    assert len(chains) >= 1000
    by_len = {k: 0 for k in (2, 3, 4, 5)}
    first, later = [0] * RL.N_PATHS, [0] * RL.N_PATHS
    dropped = real = gap = odd = 0
    for c in chains:
        by_len[min(len(c["exons"]), 5)] += 1
        for i, s in enumerate(c["steps"][1:]):
            (first if i == 0 else later)[s & 15] += 1
        dropped += c["dropped_first"]
        real += CL.is_a_chain(c["est"], gen, c["exons"], c["settings"], (c["exons_after"], c["steps"]))
        gap += CL.has_est_gap(c["exons"])
        odd += CL.odd_bases_near_a_junction(c["est"], c["exons"])
    assert min(by_len.values()) >= 150, by_len
    assert all(first[p] >= 25 for p in CL.PATHS_FIRST), first
    assert all(later[p] >= 25 for p in CL.PATHS_LATER), later
    assert first[1] == 0 and later[0] == 0
    assert dropped >= 25 and real >= 100 and gap >= 25 and odd >= 25, (dropped, real, gap, odd)
    assert os.path.getsize(CL.FIXTURE) <= os.path.getsize(RL.FIXTURE)


def test_caps_and_einval_rules_of_the_restatement():
    gen, chains = CL.load_fixture()
    c = chains[0]
    est, ex, st = c["est"], c["exons"], c["settings"]
    # a window over a cap ends the chain where it stands
    wide = (CL.MAX_EST_WINDOW + 1, st[1], st[2], st[3])
    long_est = est[:ex[0][0]] + b"ACGT" * 60 + est[ex[0][0]:]
    moved = [(ex[0][0], ex[0][1] + 240, ex[0][2], ex[0][3])] + [(e[0] + 240, e[1] + 240, e[2], e[3]) for e in ex[1:]]
    status, done, dropped, ex2, steps = CL.chain(long_est, gen, moved, wide)
    assert (status, done, dropped, ex2, steps) == (CL.ERANGE, 0, 0, moved, [0] * len(ex))
    assert CL.chain(est, gen, ex[:1], st) == (CL.OK, 0, 0, ex[:1], [0])

    def q(**kw):
        d = dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(ex), reserved=0, suffpref_length_on_est=st[0],
                 suffpref_length_for_intron=st[1], suffpref_length_on_gen=st[2], min_intron_length=st[3])
        d.update(kw)
        return d
    assert not CL.einval(len(est), len(gen), ex, [q()])
    assert not CL.einval(len(est), len(gen), ex, [q(min_intron_length=-5)])
    for bad in (q(n_exons=0), q(n_exons=len(ex) + 1), q(first_exon=1), q(est_len=len(est) + 1), q(est_off=1), q(reserved=1),
                q(suffpref_length_on_gen=-1), q(suffpref_length_for_intron=(1 << 24) + 1)):
        assert CL.einval(len(est), len(gen), ex, [bad]), bad
    assert CL.einval(len(est), len(gen), ex, [q(n_exons=2), q(first_exon=1, n_exons=len(ex) - 1)])       # a shared exon
    for k, v in ((0, -2), (1, len(est) + 1), (2, -2), (3, len(gen) + 1)):
        e2 = list(ex)
        e2[1] = tuple(v if i == k else x for i, x in enumerate(ex[1]))
        assert CL.einval(len(est), len(gen), e2, [q()])
    e2 = list(ex)
    e2[0] = (ex[0][0], ex[1][0], ex[0][2], ex[0][3])                  # my_assert of :52
    assert CL.einval(len(est), len(gen), e2, [q()])
    e2[0] = (ex[0][0], ex[0][1], ex[0][2], ex[1][2])                  # my_assert of :53
    assert CL.einval(len(est), len(gen), e2, [q()])


def test_binding_matches_the_header():
    from pintron_amd import capi
    assert "pgpu_index_refine_chains" in capi.EXPORTS and "pgpu_index_refine_chains_kernel_ms" in capi.EXPORTS
    text = open(HEADER).read()
    assert int(re.search(r"#define PGPU_CHAIN_MAX_EST_WINDOW\s+(\d+)", text).group(1)) == capi.CHAIN_MAX_EST_WINDOW == CL.MAX_EST_WINDOW >= 192
    assert int(re.search(r"#define PGPU_CHAIN_MAX_GEN_WINDOW\s+(\d+)", text).group(1)) == capi.CHAIN_MAX_GEN_WINDOW == CL.MAX_GEN_WINDOW >= 320
    assert int(re.search(r"#define PGPU_REFINE_MAX_DIM\s+(\d+)", text).group(1)) == 1024
    assert int(re.search(r"#define PGPU_REFINE_MAX_ED\s+(\d+)", text).group(1)) == 256
    for cname, struct, dtype in (("pgpu_chain_query", capi.ChainQuery, capi.CHAIN_QUERY_DTYPE),
                                 ("pgpu_chain_result", capi.ChainResult, capi.CHAIN_RESULT_DTYPE)):
        BL.assert_layout(cname, struct, dtype)
    assert np.dtype(capi.FACTOR_DTYPE).itemsize == C.sizeof(capi.Factor) == 16
