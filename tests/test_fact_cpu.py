"""CPU: the factorization stage's restatement (tests/fact_lib.py) against the host's ef_chain_factorization on real inputs,
the cover of what the GPU tests use, the hand-made cases, the binding against the header, and the host side of
pgpu_index_factorizations under the sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import cand_lib as KL
import chain_lib as RC
import fact_lib as F
import meg_lib as M
import refine_lib as RL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the host's ef_chain_factorization, the oracle as backend (ef_gpu_open over tests/hostcheck/fake_pgpu.c) ----------
class Host:
    def __init__(self, genomic: bytes):
        H = self.H = KL.host_lib()
        H.ef_gpu_open.restype = C.c_void_p
        H.ef_gpu_open.argtypes = [C.c_void_p]
        H.ef_gpu_close.argtypes = [C.c_void_p]
        H.ef_chain_factorization.restype = C.c_uint
        H.ef_chain_factorization.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_uint)]
        self.gen = C.create_string_buffer(genomic, len(genomic) + 2)
        self.seq = C.create_string_buffer(4096)                   # an ef_seq: char* id, seq, original_seq, ...; the rest 0
        struct.pack_into("<QQQ", self.seq, 0, 0, C.addressof(self.gen), C.addressof(self.gen))
        self.cfg = C.create_string_buffer(4096)
        H.ef_config_defaults(self.cfg)
        self.be = H.ef_gpu_open(self.seq)
        assert self.be

    def factorization(self, rec, est: bytes):
        """(0 not one path | 1 no factorization | 2, exons)"""
        cap = 128
        ex = (C.c_int32 * (4 * cap))()
        n = C.c_uint(0)
        kind = self.H.ef_chain_factorization(rec, self.cfg, est, self.gen, self.be, ex, cap, C.byref(n))
        assert n.value <= cap
        return kind, [tuple(ex[4 * k:4 * k + 4]) for k in range(n.value)]

    def close(self):
        self.H.ef_gpu_close(self.be)


_real = {}


def real_answers(source):
    """[(record, est, candidate, answer, info)] of one real input under the defaults, the host's graphs; computed once"""
    if source not in _real:
        gfa, efa = KL.real_inputs()[source]
        exp, genomic = M.first_attempt_megs(gfa, efa, M.DEFAULTS)
        recs, _ = KL.host_records(gfa, efa, M.DEFAULTS)
        out = []
        for e, rec in zip(exp, recs):
            est = e["seq"].encode() if isinstance(e["seq"], str) else e["seq"]
            cand = KL.candidate(rec, genomic, 15, 40)
            info = {}
            out.append((rec, est, cand, F.factorization(cand[0], est, genomic, cand[3], F.DEFAULTS, info), info))
        _real[source] = (genomic, out)
    return _real[source]


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_restatement_equals_the_host_code_on_real_inputs(source):
    genomic, rows = real_answers(source)
    host = Host(genomic)
    try:
        n_done = n_host = 0
        for k, (rec, est, cand, mine, _) in enumerate(rows):
            if mine["outcome"] == F.HOST and mine["stage"] > 0:       # a cap of the device: the host has none
                n_host += 1
                continue
            kind, exons = host.factorization(rec, est)
            want = {F.HOST: 0, F.EMPTY: 1, F.DONE: 2}[mine["outcome"]]
            assert kind == want and exons == mine["exons"], (source, k, kind, mine)
            n_done += kind == 2
        assert n_done > (len(rows) // 4 if source != "ambn" else 5) and n_host == 0, (n_done, n_host)      # (ambn: mostly no path)
    finally:
        host.close()


def cells(answers):
    return [(a["outcome"], a["stage"], a["detail"]) for a in answers]


def test_the_cover_of_what_the_gpu_tests_use():
    # the real inputs, under the defaults
    _, c2 = real_answers("c2")
    a = [r[3] for r in c2]
    done = [r for r in c2 if r[3]["outcome"] == F.DONE]
    assert len(c2) == 307 and len(done) > 307 // 4 and sum(bool(r[4].get("est_gap")) for r in done) >= 20
    assert any(x["outcome"] == F.EMPTY for x in a)
    _, i13 = real_answers("issue13")
    a = [r[3] for r in i13]
    c = cells(a)
    assert len(i13) == 1891 and sum(x["outcome"] == F.DONE for x in a) > 1891 // 4
    at_clean = [d for o, s, d in c if (o, s) == (F.EMPTY, 1)]
    assert len(at_clean) >= 25 and {4, 6, 7} <= set(at_clean)
    assert any(x["outcome"] == F.DONE and x["n_merged"] for x in a) and (F.EMPTY, 0, KL.REFUSED) in c
    assert not any(o == F.HOST and s > 0 for o, s, d in c)
    assert any(o == F.HOST and s == 0 and d == KL.NOT_PATH for o, s, d in c)
    # the three committed fixtures pushed through as candidates
    per = {}
    for name in ("clean_chains", "gap_chains", "refine_chains"):
        per[name] = [x for v in F.fixture_answers(name).values() for x in v]
    c = cells(per["clean_chains"])
    assert sum(o == F.DONE for o, _, _ in c) > 300 and {(F.EMPTY, 1, v) for v in range(1, 8)} <= set(c)
    g = per["gap_chains"]
    assert sum(x["outcome"] == F.DONE for x in g) > 600 and sum(x["outcome"] == F.DONE and x["n_merged"] > 0 for x in g) > 200
    assert cells(g).count((F.EMPTY, 2, 1)) > 150 and all(x["total_edit"] > 20 for x in g if (x["outcome"], x["stage"]) == (F.EMPTY, 2))
    r = per["refine_chains"]
    assert sum(x["outcome"] == F.DONE for x in r) > 250 and cells(r).count((F.DONE, 3, 1)) >= 3
    # nothing a fixture or a real input holds is HOST behind stage 0: those cells are the hand-made cases'
    everything = c + cells(g) + cells(r)
    assert not any(o == F.HOST for o, _, _ in everything)


def test_hand_made_cases_reach_every_host_cell_and_the_caps_last_accepted_values():
    g, cases = F.hand_cases()
    got = {}
    for name, est, ex, prm, claim in cases:
        info = {}
        a = got[name] = F.factorization(KL.ONE if ex else KL.NONE, est, g, ex, prm, info)
        cell = (a["outcome"], a["stage"], a["detail"])
        if claim is not None:
            assert cell[:2] == claim[:2] and (claim[2] is None or cell[2] == claim[2]), (name, cell)
        got[name] = (a, info, prm, est)
    seen = {(a["outcome"], a["stage"], a["detail"]) for a, _, _, _ in got.values()}
    assert {(F.HOST, 0, KL.NONE), (F.HOST, 1, 1), (F.HOST, 1, 2), (F.HOST, 2, 1), (F.HOST, 2, 2), (F.HOST, 3, 1)} <= seen
    # (HOST, 3, 2) cannot be reached: what gaps keeps is strictly ordered.  The guard stays.
    assert (F.HOST, 3, 2) not in seen
    # the caps' last accepted values pass their cap: the outcome falls behind it or not at all
    assert got["exons_64"][0]["outcome"] == F.DONE and len(got["exons_64"][0]["exons"]) == 64
    assert got["est_gap_64"][0]["outcome"] == F.DONE and got["est_gap_64"][1]["est_gap"]
    assert got["gap_p_equals_gap_t"][0]["outcome"] == F.DONE and got["gap_p_equals_gap_t"][0]["n_merged"] == 1
    # the windows of the refine cases are the sizes their names say
    for name, want in (("est_window_192", (192, None)), ("est_window_193", (193, None)), ("gen_window_320", (None, 320)),
                       ("gen_window_321", (None, 321))):
        a, info, prm, est = got[name]
        st, verdict, total, kept, after, steps = info["gaps"]
        lst = [e for e, s in zip(after, steps) if not s & F.MERGED]
        se, sg = RL.gap_windows(est, g, lst[0], lst[1], *prm[1:4])
        assert (want[0] is None or len(se) == want[0]) and (want[1] is None or len(sg) == want[1]), (name, len(se), len(sg))
        assert len(se) <= RC.MAX_EST_WINDOW or want[0] == 193
    # what an end exon of 4 096 bytes asks of the workspace: the largest a call can need
    a, info, prm, est = got["end_exon_4096"]
    assert info["clean"][0] == F.OK


def test_nothing_reaches_the_guard_behind_gaps():
    """what gaps keeps is strictly ordered on both strings, whatever it was given: every list the
    restatement sends through check_gap_errors with verdict 0 -- on the three fixtures, the real inputs and the hand-made
    cases -- and every recorded answer of the gap_chains fixture"""
    import gaps_lib as GL

    def ordered(after, steps):
        lst = [e for e, s in zip(after, steps) if not s & F.MERGED]
        return all(d[1] < a[0] and d[3] < a[2] for d, a in zip(lst, lst[1:]))

    infos = [i for name in ("clean_chains", "gap_chains", "refine_chains") for v in F.fixture_infos(name).values() for i in v]
    infos += [r[4] for src in ("c2", "ambn", "issue13") for r in real_answers(src)[1]]
    g, cases = F.hand_cases()
    for name, est, ex, prm, claim in cases:
        info = {}
        F.factorization(KL.ONE if ex else KL.NONE, est, g, ex, prm, info)
        infos.append(info)
    n = 0
    for info in infos:
        if "gaps" in info and info["gaps"][0] == F.OK and info["gaps"][1] == 0:
            assert ordered(info["gaps"][4], info["gaps"][5])
            n += 1
    assert n > 2500, n
    gen, cases = GL.load_fixture()
    assert all(ordered(c["exons_after"], c["steps"]) for c in cases if c["verdict"] == 0)


def test_binding_matches_the_header():
    from pintron_amd import capi
    names = ["pgpu_pairing_plan_run_factorizations", "pgpu_pairing_plan_factorization_exons", "pgpu_pairing_plan_fetch_factorizations",
             "pgpu_pairing_plan_factorizations_ms", "pgpu_index_factorizations", "pgpu_index_factorizations_kernel_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(capi.EXPORTS) == sorted(set(re.findall(r"\b(pgpu_[a-z_0-9]+)\s*\(", hdr)))
    import binding_lib as B
    B.assert_layout("pgpu_fact_params", capi.FactParams, capi.FACT_PARAMS_DTYPE)
    # pgpu_fact_result has 8- and 16-bit fields
    size_of = dict(B.SIZE_OF, uint16_t=2, uint8_t=1)
    fields, size = B.header_struct("pgpu_fact_result")
    import numpy as np
    dt = np.dtype(capi.FACT_RESULT_DTYPE)
    assert [f for f, _ in fields] == [f for f, _ in capi.FactResult._fields_] == [f for f, _ in capi.FACT_RESULT_DTYPE]
    off = 0
    for f, ctype in fields:
        assert getattr(capi.FactResult, f).offset == off == dt.fields[f][1], f
        assert getattr(capi.FactResult, f).size == size_of[ctype] == dt.fields[f][0].itemsize, f
        off += size_of[ctype]
    assert off == size == 16 == C.sizeof(capi.FactResult) == dt.itemsize
    assert re.search(r"typedef pgpu_gaps_query pgpu_fact_query;", text) and capi.FactQuery is capi.GapsQuery
    for k, name in enumerate(("HOST", "EMPTY", "DONE")):
        assert re.search(r"#define PGPU_FACT_%s\s+%du\b" % (name, k), text) and getattr(capi, "FACT_" + name) == getattr(F, name) == k
    # the defaults of the bindings and of the restatement are est-fact's (pintron_amd/host/ef_config.c)
    import inspect
    src = open(os.path.join(ROOT, "pintron_amd", "host", "ef_config.c")).read()
    conf = {k: float(v) for k, v in re.findall(r"c->(complexity_threshold|suffpref_length_on_est|suffpref_length_for_intron|"
                                               r"suffpref_length_on_gen|min_intron_length) = ([0-9.]+);", src)}
    want = (conf["complexity_threshold"], conf["suffpref_length_on_est"], conf["suffpref_length_for_intron"],
            conf["suffpref_length_on_gen"], conf["min_intron_length"])
    assert F.DEFAULTS == want
    for fn in (capi.Index.factorizations, capi.PairingPlan.run_factorizations):
        assert tuple(p.default for p in inspect.signature(fn).parameters.values() if p.default is not inspect.Parameter.empty) == want


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fact_call_check")                      # pgpu_fact.h needs the C-ABI's header alone: no ROCm header
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "hostcheck", "fact_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
