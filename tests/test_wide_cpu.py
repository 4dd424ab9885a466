"""CPU: the wide restatement (tests/wide_lib.py) against the fixture that the reference's object code, the restatement and
the host's ef_chain_tail / ef_chain_small agreed on (tests/golden/wide_chains.json.gz), the fixture's cover, that the wide
restatement is the narrow one wherever the narrow one answers, the real inputs, two broken restatements the fixture
notices, the bindings and the header's constants.

On c2, test-AMBN and test-issue-13 no one-path record flips: none is HOST for a window cap under the narrow final and settled
under the wide one (counted below: 0, 0 and 0 at the default settings and with min_intron_length 4; one pattern of
test-issue-13 passes the tail stage's cap under the wide form and is then refused by the small stage).  So these inputs show
only that the wide final equals the narrow one wherever no window cap is met; the hand-made cases carry the floor."""
import re

import pytest

import cand_lib as KL
import fact_lib as F
import final_lib as FL
import small_lib as SL
import tail_lib as TL
import test_fact_cpu as TF
import wide_lib as WL


def test_the_wide_restatement_equals_the_fixture():
    gen, tails, smalls = WL.load_fixture()
    assert len(tails) >= 150 and len(smalls) >= 100
    for c in tails:
        info = {}
        got = WL.tail(c["orig"], c["est"], gen, c["exons"], info=info)
        assert got == c["answer"], c["name"]
        assert WL.tail_tags(c["orig"], c["est"], gen, c["exons"], got, info) == c["tags"], c["name"]
    ops = SL.OracleOps(gen)
    for c in smalls:
        got = WL.small(c["orig"], c["est"], gen, c["exons"], c["mil"], ops=ops)
        assert got == c["answer"], c["name"]
        assert c["witnesses"] == [1, 2, 3], c["name"]
    assert TL.MAX_AFFIX == 256 and SL.MAX_PREFIX_WINDOW == 256            # restored behind every call


def test_the_fixtures_cover():
    gen, tails, smalls = WL.load_fixture()
    count = {t: 0 for t in WL.TAGS}
    for c in tails + smalls:
        assert c["tags"] <= set(WL.TAGS), c["name"]
        for t in c["tags"]:
            count[t] += 1
    assert min(count.values()) >= WL.MIN_PER_TAG, count
    md = open(WL.FIXTURE[:-len(".json.gz")] + ".md").read()
    assert {t: int(n) for t, n in re.findall(r"`(\w+)`: (\d+)", md.split("- cover (cases):")[1].split("\n")[0])} == count
    # what each length must be: answered up to 1024 (the skipped ones at any length), refused beyond
    for c in tails:
        (pe, _, pa), (se, _, sa) = WL.tail_windows(c["est"], gen, c["exons"])
        over = (pa and pe > WL.TAIL_WIDE_MAX_AFFIX) or (sa and se > WL.TAIL_WIDE_MAX_AFFIX)
        assert (c["answer"][0] == TL.ERANGE) == (over or "tail_other_cap" in c["tags"]), c["name"]
    by = lambda t: [c for c in smalls if t in c["tags"]]
    assert all(c["answer"][:2] == (SL.ERANGE, 2) for c in by("window_1025"))
    assert all(c["answer"][:2] == (SL.ERANGE, 4) for c in by("small_other_cap"))
    assert all(c["answer"][0] == SL.OK for w in WL.WIDTHS[:-1] for c in by("window_%d" % w) if "small_other_cap" not in c["tags"])
    for w in WL.WIDTHS[1:-1]:                                               # at every wide length both outcomes of the search
        assert {c["answer"][3] for c in by("window_%d" % w)} == {0, 1}, w
    # the narrow restatement refuses every case tagged wide whose question runs
    ops = SL.OracleOps(gen)
    for c in tails:
        if c["tags"] & {"pre_wide", "suf_wide"}:
            assert TL.tail(c["orig"], c["est"], gen, c["exons"])[0] == TL.ERANGE, c["name"]
        elif c["answer"][0] == TL.OK:
            assert TL.tail(c["orig"], c["est"], gen, c["exons"]) == c["answer"], c["name"]
    for c in smalls:
        if c["tags"] & {"wide_inserted", "wide_not_inserted", "small_other_cap", "window_1025"}:
            assert SL.small(c["orig"], c["est"], gen, c["exons"], c["mil"], ops=ops)[:2] == (SL.ERANGE, 2), c["name"]


def test_wide_equals_narrow_wherever_narrow_answers_on_the_two_fixtures():
    gen, cases, _ = TL.load_fixture()
    n = 0
    for c in cases:
        wide = WL.tail(c["orig"], c["est"], gen, c["exons"])
        if "affix_257" in c["tags"]:                                        # the narrow cap's own refusals: 257 bytes are answered
            assert c["answer"][0] == TL.ERANGE and wide[0] == TL.OK, c["name"]
        else:
            assert wide == c["answer"], c["name"]
            n += 1
    assert n >= 400, n
    n = 0
    for g, cases in SL.load_fixture()[0]:
        ops = SL.OracleOps(g)
        for c in cases:
            wide = WL.small(c["orig"], c["est"], g, c["exons"], c["mil"], ops=ops)
            if c["answer"][:2] != (SL.ERANGE, 2):
                assert wide == c["answer"], c["name"]
                n += 1
            else:
                assert wide[:2] != (SL.ERANGE, 2), c["name"]
    assert n >= 100, n


REAL_FLIPS = {"c2": 0, "ambn": 0, "issue13": 0}       # one-path records HOST for a window cap under the narrow final, not under the wide


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_real_inputs_flipped_records_equal_the_host_code(source):
    genomic, rows = TF.real_answers(source)
    host, ops = SL.Host(genomic), SL.OracleOps(genomic)
    flips = 0
    try:
        for k, (rec, est, cand, _, _) in enumerate(rows):
            if cand[0] not in (KL.ONE, KL.REFUSED):
                continue
            for mil in (int(F.DEFAULTS[4]), 4):
                narrow = FL.final(cand[0], est, est, genomic, cand[3], F.DEFAULTS, mil, ops=ops)
                for_window = narrow["outcome"] == FL.HOST and narrow["detail"] == 1 and \
                    (narrow["stage"] == 4 or (narrow["stage"] == 5 and narrow["refused"] == 2))
                info = {}
                wide = WL.final(cand[0], est, est, genomic, cand[3], F.DEFAULTS, mil, ops=ops, info=info)
                if not for_window:
                    assert wide == narrow, (source, k, mil)
                    continue
                if wide["outcome"] == FL.HOST:
                    continue
                flips += 1
                host._set_mil(int(F.DEFAULTS[4]))
                kind, exons = host.factorization(rec, est)
                assert kind == 2, (source, k)
                dropped, polyA, polyadenil, left = host.tail(est, est, exons)
                assert (polyA, polyadenil) == (wide["polyA"], wide["polyadenil"]), (source, k)
                if (wide["outcome"], wide["stage"]) == (FL.EMPTY, 4):
                    assert dropped == 1, (source, k)
                    continue
                assert dropped == 0 and left == TL.kept_exons(info["tail_answer"]), (source, k)
                if info["small"].get("outside"):
                    continue
                emptied, final = host.small(est, est, left, mil)
                if wide["outcome"] == FL.EMPTY:
                    assert emptied == 1, (source, k, mil)
                else:
                    assert emptied == 0 and final == [tuple(e) for e in wide["exons"]], (source, k, mil)
    finally:
        host.close()
    assert flips == REAL_FLIPS[source], flips


def test_the_fixture_notices_a_cap_of_512_and_a_genomic_window_cut_at_304():
    gen, tails, smalls = WL.load_fixture()
    ops = SL.OracleOps(gen)
    with WL.caps(512, 512):
        at_512 = sum(TL.tail(c["orig"], c["est"], gen, c["exons"]) != c["answer"] for c in tails)
        at_512_small = sum(SL.small(c["orig"], c["est"], gen, c["exons"], c["mil"], ops=ops) != c["answer"] for c in smalls)
    assert at_512 >= WL.MIN_PER_TAG and at_512_small >= WL.MIN_PER_TAG, (at_512, at_512_small)
    cut = sum(WL.tail(c["orig"], c["est"], gen, c["exons"], ops=WL.Cut304Ops()) != c["answer"] for c in tails)
    assert cut >= WL.MIN_PER_TAG, cut


def test_bindings_exports_and_the_headers_constants():
    import inspect
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_index_tail_chains_wide", "pgpu_index_small_chains_wide", "pgpu_index_final_factorizations_wide",
             "pgpu_pairing_plan_run_final_factorizations_wide"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    for wide, narrow in zip(names, (n[:-len("_wide")] for n in names)):
        assert getattr(L, wide).argtypes == getattr(L, narrow).argtypes, wide
    for cls, method in ((capi.Index, "tail_chains_raw"), (capi.Index, "tail_chains"), (capi.Index, "small_chains_raw"),
                        (capi.Index, "small_chains"), (capi.Index, "final_factorizations_raw"), (capi.Index, "final_factorizations"),
                        (capi.PairingPlan, "run_final_factorizations_raw"), (capi.PairingPlan, "run_final_factorizations")):
        assert inspect.signature(getattr(cls, method)).parameters["wide"].default is False, method
    text = open(B.HEADER).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(PGPU_\w+)\s+(\d+)\b", text)}
    assert defs["PGPU_TAIL_WIDE_MAX_AFFIX"] == WL.TAIL_WIDE_MAX_AFFIX == 1024
    assert defs["PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW"] == WL.SMALL_WIDE_MAX_PREFIX_WINDOW == 1024
    assert defs["PGPU_TAIL_MAX_AFFIX"] == WL.NARROW_MAX_AFFIX == TL.MAX_AFFIX
    assert defs["PGPU_SMALL_MAX_PREFIX_WINDOW"] == WL.NARROW_MAX_PREFIX_WINDOW == SL.MAX_PREFIX_WINDOW
    assert int(1.17 * defs["PGPU_TAIL_WIDE_MAX_AFFIX"]) == WL.WIDE_AFFIX_GEN == 1198
