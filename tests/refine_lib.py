"""CPU restatement of the intron-border decision (pgpu_index_refine_introns) with the branch that decided.

refine          refine_intron (src/refine-intron.c:47-265) from the gap alignment onward, as
                pintron_amd/host/ef_refine_intron.c:455-509 restates it with find_*, shift_generic and
                try_burset_after_match, written out once more in plain Python: one query in, (status, refined, path,
                donor, acceptor) out.  Outside the reference's domain the definition is the header's: a row byte
                outside [0, dim) reads as 0, a NUL inside a row ends it, a byte of the EST or of the genomic sequence
                outside the string reads as 0 (the terminator).
RefRefiner      refine_intron of the reference's own object code through ctypes (oracle/_ref), where it exists.
load_fixture    tests/golden/refine_introns.json.gz (tools/make_refine_golden.py).
make_case / random_queries   generated workloads: introns planted in a sequence, borders moved, sites of every kind.
"""
import ctypes as C
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "refine_introns.json.gz")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libpintron_ref_core.so")

MAX_DIM = 1024            # PGPU_REFINE_MAX_DIM
MAX_ED = 256              # PGPU_REFINE_MAX_ED
OK, ERANGE = 0, -34
PATH_NAMES = ["attached-first", "attached-later", "too-small", "shift>20", "canonical", "r2l_1", "l2r_1", "r2l_2", "l2r_2",
              "burset"]
N_PATHS = 10
GAP = 45                  # '-'
U32 = 0xFFFFFFFF


def burset_table():
    """the 256 frequencies of getBursetFrequency as data, read out of the product's host file"""
    import re
    text = open(os.path.join(ROOT, "pintron_amd", "host", "ef_refine_intron.c")).read()
    m = re.search(r"burset_tab\[256\]\s*=\s*\{(.*?)\};", text, re.S)
    tab = [int(x) for x in re.findall(r"\d+", m.group(1))]
    assert len(tab) == 256
    return tab


_BURSET = None
_CODE = {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}


def burset_frequency(d: bytes, a: bytes) -> int:
    global _BURSET
    if _BURSET is None:
        _BURSET = burset_table()
    if len(d) != 2 or len(a) != 2:
        return 0
    c = [_CODE.get(x, -1) for x in d + a]
    if min(c) < 0:
        return 0
    return _BURSET[(c[0] << 6) | (c[1] << 4) | (c[2] << 2) | c[3]]


def substring(s: bytes, index: int, length: int) -> bytes:
    """real_substring (src/util.c:138-158): clamped at the start, cut at the terminator"""
    if index < 0:
        length += index
        index = 0
    if length < 0:
        length = 0
    out = s[index:index + length]
    z = out.find(b"\0")
    return out if z < 0 else out[:z]


def check_burset_patterns(gen: bytes, donor_left: int, acceptor_right: int) -> int:
    return burset_frequency(substring(gen, donor_left + 1, 2), substring(gen, acceptor_right - 2, 2))


class Aln:
    """the two rows and v[1..5]; byte access with the header's out-of-range rule"""

    def __init__(self, est_row: bytes, gen_row: bytes, factor_cut, intron_start, intron_end, isoa, ieoa):
        assert len(est_row) == len(gen_row)
        self.dim = len(gen_row)
        self.e, self.g = est_row, gen_row
        self.factor_cut, self.intron_start, self.intron_end, self.isoa, self.ieoa = factor_cut, intron_start, intron_end, isoa, ieoa
        z = gen_row.find(b"\0")
        self.glen = self.dim if z < 0 else z
        z = est_row.find(b"\0")
        self.elen = self.dim if z < 0 else z

        self.outside = False          # a scan has read a row in front of its first byte or behind its terminator

    def G(self, i):
        if 0 <= i < self.dim:
            return self.g[i]
        self.outside |= i != self.dim
        return 0

    def E(self, i):
        if 0 <= i < self.dim:
            return self.e[i]
        self.outside |= i != self.dim
        return 0


def find_AG_after_right(al, init):
    """Find_AG_after_on_the_right (:892-940) -> (cut_on_align, gen_cut, est_cut)"""
    index = init - 2
    if index < 0 or al.glen == 0:              # (size_t)(init - 2) is beyond every row; an empty row has nothing to find
        return -1, -1, -1
    stop = False
    while not stop and index < al.glen - 1:
        while al.G(index) == GAP:
            index += 1
        p0 = al.G(index)
        index += 1
        while al.G(index) == GAP:
            index += 1
        stop = p0 == 65 and al.G(index) == 71
    if not stop:
        return -1, -1, -1
    cg = ce = 0
    for i in range(al.ieoa + 1, index + 1):
        cg += al.G(i) != GAP
        ce += al.E(i) != GAP
    return index + 1, cg, ce


def find_before_left(al, init, pat):
    """Find_ACCEPTOR_before_on_the_left (:942-990) -> (cut_on_align, gen_cut, est_cut)"""
    index = init + 2
    stop = False
    while not stop and index > 0:
        while al.G(index) == GAP:
            index -= 1
        p1 = al.G(index)
        index -= 1
        while index >= 0 and al.G(index) == GAP:
            index -= 1
        p0 = 0 if index < 0 else al.G(index)
        stop = p0 == pat[0] and p1 == pat[1]
    if not stop:
        return -1, -1, -1
    cg = ce = 0
    for i in range(al.isoa - 1, index - 1, -1):
        cg += al.G(i) != GAP
        ce += al.E(i) != GAP
    return index - 1, cg, ce


def find_after_left(al, init, pat):
    """Find_ACCEPTOR_after_on_the_left (:1852-1874) -> substr_dim"""
    index = init
    stop = False
    while not stop and index < al.ieoa:
        p0 = al.G(index)
        index += 1
        stop = p0 == pat[0] and al.G(index) == pat[1]
    return index - al.isoa - 1 if stop else -1


def find_AG_before_right(al, init):
    """Find_AG_before_on_the_right (:1950-1972) -> substr_dim"""
    index = init
    stop = False
    while not stop and index > al.isoa:
        p1 = al.G(index)
        index -= 1
        stop = al.G(index) == 65 and p1 == 71
    return al.ieoa - index - 1 if stop else -1


def row_substring(al, genomic, init, length):
    """Get_genomic/est_substring_from_alignment (:1878-1948) -> (string, mismatches) or None"""
    if init < 0 or init >= al.glen:
        return None
    rlen = al.glen if genomic else al.elen
    actual = min(rlen - init, length)
    row = al.G if genomic else al.E
    out, herr = bytearray(), 0
    for i in range(init, init + actual):
        if row(i) != GAP:
            out.append(row(i))
        herr += al.G(i) != al.E(i)
    return bytes(out), herr


STATS = {"wrapped": 0}       # how often the unsigned difference of the _1 rule went below zero (the tests ask)


class TooLong(Exception):
    pass


def levenshtein(a: bytes, b: bytes) -> int:
    """PGPU_DP_ED: plain Levenshtein, N is no wildcard; an operand beyond the cap refuses the query"""
    if len(a) > MAX_ED or len(b) > MAX_ED:
        raise TooLong()
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[len(b)]


def shift_generic(est, gen, al, naf, ndr, nalg, r2l, variant1, pat):
    """the common body of the four Shift_* routines (:992-1850) -> (settled, donor_right, acc_left, factor_left)"""
    init_right = al.ieoa + 1 if r2l else al.ieoa
    init_left = al.isoa if r2l else al.isoa - 1
    ext_error = -1
    if r2l:
        l_substr, start = 8, al.isoa - 8
        if start < 0:
            l_substr, start = l_substr - start, 0
    else:
        l_substr, start = 8, al.ieoa + 1
    xe, xg = row_substring(al, False, start, l_substr), row_substring(al, True, start, l_substr)
    ext_est = ext_gen = None
    if xe is not None:
        ext_est, ext_error = xe
    if xg is not None:
        ext_gen, ext_error = xg
    gen_cut, est_cut, sub_dim = [0, 0], [0, 0], [0, 0]
    cut_factor, match_str, prev_match, ext_cut, ext_match = ([None, None] for _ in range(5))
    for i in range(2):
        if r2l:
            cut_on_align, gen_cut[i], est_cut[i] = find_AG_after_right(al, init_right)
        else:
            cut_on_align, gen_cut[i], est_cut[i] = find_before_left(al, init_left, pat)
        if est_cut[i] > -1:
            if r2l:
                prev_match[i] = substring(gen, nalg, gen_cut[i])
                cut_factor[i] = substring(est, naf, est_cut[i])
                init_right = cut_on_align + 1
            else:
                prev_match[i] = substring(gen, ndr - gen_cut[i] + 1, gen_cut[i])
                cut_factor[i] = substring(est, naf - est_cut[i], est_cut[i])
                init_left = cut_on_align - 1
            if ext_error > 0 and ext_est is not None:
                ext_cut[i] = ext_est + cut_factor[i] if r2l else cut_factor[i] + ext_est
        sub_dim[i] = find_after_left(al, init_left, pat) if r2l else find_AG_before_right(al, init_right)
        if sub_dim[i] > -1:
            if r2l:
                match_str[i] = substring(gen, ndr + 1, sub_dim[i])
                init_left = al.isoa + sub_dim[i] + 1
            else:
                match_str[i] = substring(gen, nalg - sub_dim[i], sub_dim[i])
                init_right = al.ieoa - sub_dim[i] - 1
            if cut_factor[i] is not None and ext_error > 0 and ext_gen is not None:
                ext_match[i] = ext_gen + match_str[i] if r2l else match_str[i] + ext_gen
    # every distance the decision can ask for, together (the grouping of ef_refine_intron.c:262-288)
    ed_prev, ed_pair = [0, 0], [[0, 0], [0, 0]]
    for i in range(2):
        if variant1 and cut_factor[i] is not None:
            ed_prev[i] = levenshtein(cut_factor[i], prev_match[i])
        for j in range(2):
            if ext_cut[i] is not None and ext_match[j] is not None:
                ed_pair[i][j] = levenshtein(ext_cut[i], ext_match[j])
            elif cut_factor[i] is not None and match_str[j] is not None:
                ed_pair[i][j] = levenshtein(cut_factor[i], match_str[j])

    def outputs(i, j):
        if r2l:
            return ndr + sub_dim[j], nalg + gen_cut[i], naf + est_cut[i]
        return ndr - gen_cut[i], nalg - sub_dim[j], naf - est_cut[i]
    out = (0, 0, 0)
    stop = False
    if variant1:
        error = edit_prev = 1000                     # unsigned in the reference: they wrap
        for i in range(2):
            for j in range(2):
                if stop:
                    break
                if cut_factor[i] is not None and match_str[j] is not None:
                    edit_prev = ed_prev[i]
                    if edit_prev <= 5:
                        if ext_cut[i] is not None and ext_match[j] is not None:
                            raw = ed_pair[i][j] - edit_prev - ext_error
                        else:
                            raw = ed_pair[i][j] - edit_prev
                        STATS["wrapped"] += raw < 0
                        error = raw & U32
                if error <= 1:
                    out = outputs(i, j)
                    stop = True
    else:
        error = 1000
        for i in range(2):
            for j in range(2):
                if stop:
                    break
                if ext_cut[i] is not None and ext_match[j] is not None:
                    edit = ed_pair[i][j] - ext_error
                elif cut_factor[i] is not None and match_str[j] is not None:
                    edit = ed_pair[i][j]
                else:
                    edit = 1000
                if edit < error:
                    error = edit
                    out = outputs(i, j)
                if error == 0:
                    stop = True
    return (stop,) + out


def try_burset_after_match(est, gen, factor_left, donor_right, acc_left, donor_factor_left, acc_factor_right):
    """Try_Burset_after_match (:267-344) -> (factor_left, donor_right, acc_left)"""
    def E(i):
        return est[i] if 0 <= i < len(est) else 0

    def Gn(i):
        return gen[i] if 0 <= i < len(gen) else 0
    z = est.find(b"\0")
    el = len(est) if z < 0 else z
    gl = len(gen)
    sf, sa, sd = factor_left, acc_left, donor_right
    uf, ua, ud = sf, sa, sd
    frequency, right_to_left, stop = 0, False, False
    while not stop and E(sf) == Gn(sa) and sf > donor_factor_left + 1:
        if sf == 0 or sd == -1:
            stop = True
        else:
            f = check_burset_patterns(gen, sd, sa)
            if f > frequency:
                frequency, uf, ua, ud = f, sf, sa, sd
            sf, sd, sa = sf - 1, sd - 1, sa - 1
    sf, sa, sd = factor_left, acc_left + 1, donor_right + 1
    stop = False
    while not stop and E(sf) == Gn(sd) and sf < acc_factor_right:
        if sf == el or sa == gl:
            stop = True
        else:
            f = check_burset_patterns(gen, sd, sa)
            if f > frequency:
                frequency, uf, ua, ud, right_to_left = f, sf, sa, sd, True
            sf, sd, sa = sf + 1, sd + 1, sa + 1
    if right_to_left:
        uf += 1
    return uf, ud, ua


def refine(est: bytes, gen: bytes, est_row: bytes, gen_row: bytes, v, donor, acceptor, first_intron, sp_est, sp_int, sp_gen,
           min_intron_length, info=None):
    """One query.  `info` (a dict) receives "outside": a scan left the rows, where the reference is not defined.  v = (factor_cut, intron_start, intron_end, intron_start_on_align, intron_end_on_align); donor and
    acceptor are (EST_start, EST_end, GEN_start, GEN_end).  -> (status, refined, path, donor, acceptor)"""
    donor, acceptor = tuple(donor), tuple(acceptor)
    if len(gen_row) > MAX_DIM:
        return ERANGE, 0, 0, donor, acceptor
    al = Aln(est_row, gen_row, *v)
    try:
        return _refine(est, gen, al, donor, acceptor, first_intron, sp_est, sp_int, sp_gen, min_intron_length)
    finally:
        if info is not None:
            info["outside"] = al.outside


def _refine(est, gen, al, donor, acceptor, first_intron, sp_est, sp_int, sp_gen, min_intron_length):
    d_es, d_ee, d_gs, d_ge = donor
    a_es, a_ee, a_gs, a_ge = acceptor
    dsl_gen = d_gs if d_ge - sp_gen + 1 < d_gs else d_ge - sp_gen + 1
    dsl_est = d_es if d_ee - sp_est + 1 < d_es else d_ee - sp_est + 1
    deleted = a_gs - d_ge - 1 - 2 * sp_int
    naf = dsl_est + al.factor_cut
    ndr = dsl_gen + al.intron_start - 1
    nalg = dsl_gen + al.intron_end + deleted + 1
    if naf == d_es:
        if first_intron:
            return OK, 1, 0, donor, (naf, a_ee, nalg, a_ge)
        return OK, 0, 1, donor, acceptor
    if nalg - ndr < min_intron_length:
        return OK, 0, 2, donor, acceptor
    if abs(ndr - d_ge) > 20 or abs(nalg - a_gs) > 20:
        return OK, 0, 3, donor, acceptor
    _, lg, _ = find_before_left(al, al.isoa - 1, b"GT")
    _, rg, _ = find_AG_after_right(al, al.ieoa + 1)
    if lg == 0 and rg == 0:
        path, fd, fa, ff = 4, ndr, nalg, naf
    else:
        try:
            for path, (r2l, v1, pat) in enumerate(((True, True, b"GT"), (False, True, b"GT"), (True, False, b"GC"),
                                                   (False, False, b"GC")), 5):
                ok, fd, fa, ff = shift_generic(est, gen, al, naf, ndr, nalg, r2l, v1, pat)
                if ok:
                    break
            else:
                path = 9
                ff, fd, fa = try_burset_after_match(est, gen, naf, ndr, nalg, d_es, a_ee)
        except TooLong:
            return ERANGE, 0, 0, donor, acceptor
        if fa > a_ge or fd < d_gs:
            return OK, 0, path, donor, acceptor
    return OK, 1, path, (d_es, ff - 1, d_gs, fd), (ff, a_ee, fa, a_ge)


# ---- the windows and the alignment a caller makes first ------------------------------------------------------------
def gap_windows(est, gen, donor, acceptor, sp_est, sp_int, sp_gen):
    """the two strings of the gap alignment (:55-108), as ef_gap_window_build"""
    d_es, d_ee, d_gs, d_ge = donor
    a_es, a_ee, a_gs, a_ge = acceptor
    dsl_gen = d_gs if d_ge - sp_gen + 1 < d_gs else d_ge - sp_gen + 1
    dsl_est = d_es if d_ee - sp_est + 1 < d_es else d_ee - sp_est + 1
    apr_gen = a_ge if a_gs + sp_gen - 1 > a_ge else a_gs + sp_gen - 1
    apr_est = a_ee if a_es + sp_est - 1 > a_ee else a_es + sp_est - 1
    se = substring(est, dsl_est, d_ee - dsl_est + 1)
    if d_ee != a_es - 1:
        se += substring(est, d_ee + 1, a_es - d_ee - 1)
    se += substring(est, a_es, apr_est - a_es + 1)
    sg = substring(gen, dsl_gen, d_ge - dsl_gen + 1) + substring(gen, d_ge + 1, sp_int) + \
        substring(gen, a_gs - sp_int, sp_int) + substring(gen, a_gs, apr_gen - a_gs + 1)
    return bytes(se), bytes(sg)


def oracle_rows(O, est, gen, donor, acceptor, sp_est, sp_int, sp_gen):
    """(est_row, gen_row, v[1..5]) from the oracle's CPU gap alignment (pinned to the reference)"""
    se, sg = gap_windows(est, gen, donor, acceptor, sp_est, sp_int, sp_gen)
    r = O.gap_align(se, sg)
    return r["ea"], r["ga"], (r["factor_cut"], r["intron_start"], r["intron_end"], r["intron_start_on_align"],
                              r["intron_end_on_align"])


# ---- the reference's object code -----------------------------------------------------------------------------------
class _RefConfig(C.Structure):       # struct _configuration (include/configuration.h:39-135): the fields by name
    _fields_ = [("min_factor_len", C.c_uint), ("min_intron_length", C.c_int), ("max_intron_length", C.c_int),
                ("min_string_depth_rate", C.c_double), ("max_prefix_discarded_rate", C.c_double),
                ("max_suffix_discarded_rate", C.c_double), ("max_prefix_discarded", C.c_int), ("max_suffix_discarded", C.c_int),
                ("max_site_difference", C.c_uint), ("max_number_of_factorizations", C.c_int), ("max_coverage_diff", C.c_double),
                ("max_exonNUM_diff", C.c_int), ("max_gapLength_diff", C.c_int), ("retain_externals", C.c_char),
                ("max_pairings_in_MEG", C.c_uint), ("max_freq_shortest_pairing", C.c_double),
                ("suffpref_length_on_est", C.c_int), ("suffpref_length_for_intron", C.c_int), ("suffpref_length_on_gen", C.c_int),
                ("trans_red", C.c_bool), ("short_edge_comp", C.c_bool), ("max_single_factorization_time", C.c_uint),
                ("complexity_threshold", C.c_double)]


class _RefFactor(C.Structure):
    _fields_ = [("EST_start", C.c_int), ("EST_end", C.c_int), ("GEN_start", C.c_int), ("GEN_end", C.c_int)]


def have_ref():
    return os.path.exists(REF_LIB)


class RefRefiner:
    """refine_intron (src/refine-intron.c:47) of the reference's object code on one genomic sequence"""

    def __init__(self, gen: bytes):
        self.L = C.CDLL(REF_LIB)
        self.L.refine_intron.restype = C.c_bool
        self.L.refine_intron.argtypes = [C.c_void_p] * 4 + [C.c_void_p, C.c_bool]
        self.gen = C.create_string_buffer(gen)
        # struct _EST_info (include/types.h:140-): refine_intron reads EST_seq alone, the second pointer
        self.gi = (C.c_void_p * 32)()
        self.gi[1] = C.addressof(self.gen)

    def refine(self, est: bytes, donor, acceptor, first_intron, sp_est, sp_int, sp_gen, min_intron_length):
        cfg = _RefConfig()
        cfg.suffpref_length_on_est, cfg.suffpref_length_for_intron, cfg.suffpref_length_on_gen = sp_est, sp_int, sp_gen
        cfg.min_intron_length = min_intron_length
        eb = C.create_string_buffer(est)
        ei = (C.c_void_p * 32)()
        ei[1] = C.addressof(eb)
        d, a = _RefFactor(*donor), _RefFactor(*acceptor)
        r = self.L.refine_intron(C.byref(cfg), C.addressof(self.gi), C.addressof(ei), C.byref(d), C.byref(a), bool(first_intron))
        return int(bool(r)), (d.EST_start, d.EST_end, d.GEN_start, d.GEN_end), (a.EST_start, a.EST_end, a.GEN_start, a.GEN_end)


    def refine_isolated(self, *args):
        """the same in a forked child: the reference's Shift_* routines overrun heap blocks on some inputs, and the
        damage shows calls later.  None when the child does not survive the call."""
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            try:
                os.close(r)
                os.write(w, json.dumps(self.refine(*args)).encode())
            finally:
                os._exit(0)
        os.close(w)
        data = b""
        while True:
            chunk = os.read(r, 65536)
            if not chunk:
                break
            data += chunk
        os.close(r)
        _, st = os.waitpid(pid, 0)
        if st != 0 or not data:
            return None
        refined, d, a = json.loads(data)
        return refined, tuple(d), tuple(a)


# ---- generated inputs ----------------------------------------------------------------------------------------------
GEN_LEN = 1_600_000


def fixture_genomic():
    """the sequence the fixture's introns are planted in, one after the other: seeded random ACGT"""
    return rnd(np.random.default_rng(303), GEN_LEN)


def rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


SITES = [(b"GT", b"AG")] * 5 + [(b"GC", b"AG")] * 3 + [(b"AT", b"AC"), (b"GG", b"AG"), (b"GT", b"GG"), (b"GA", b"TG"),
                                                       (b"CT", b"AC"), None, None]


def make_case(rng, p, site="rand", short_exons=False, aim=None):
    """One planted intron whose donor exon starts at `p`: the positions of the two exons and `edits` = [(pos, bytes)],
    the sites to write into the sequence first."""
    l1, l2 = int(rng.integers(34, 60)), int(rng.integers(34, 60))
    if short_exons:                                 # one exon of a few bases: a shifted border can leave it
        if rng.random() < 0.5:
            l1 = int(rng.integers(3, 12))
        else:
            l2 = int(rng.integers(3, 12))
    k = int(rng.integers(2, 7))
    if aim == "attached":
        l1 = int(rng.integers(3, 11))
    elif aim == "refused-acceptor":
        l2 = k + 2
    elif aim == "refused-donor":
        l1 = k + 2
    ilen = int(rng.integers(60, 200)) if rng.random() < 0.7 else int(rng.integers(200, 800))
    ds, de = p, p + l1 - 1                          # donor exon on the sequence, inclusive
    as_, ae = de + 1 + ilen, de + ilen + l2
    edits = []
    if site == "rand":
        site = SITES[int(rng.integers(len(SITES)))]
    if site is not None:
        edits += [(de + 1, site[0]), (as_ - 2, site[1])]
    t = rnd(rng, k)
    d2 = site[0] if site is not None else b"GC"
    if aim == "repeat-left":          # the intron begins as the acceptor exon does: the alignment may cut behind the true site
        edits += [(de + 1, d2 + t), (as_, d2 + t)]
    elif aim == "repeat-right":       # the donor exon ends as the intron does: it may cut in front of it
        edits += [(de - k - 1, t + b"AG"), (as_ - k - 2, t + b"AG")]
    elif aim == "gc-left":            # a GC-AG intron k bases to the left of a junction without sites, the same bases at both
        edits += [(de + 1, b"CC"), (de - k - 1, b"GC" + t), (as_ - k - 4, b"AG" + b"GC" + t)]
    elif aim == "refused-acceptor":   # the whole acceptor exon can move in front of the intron
        edits += [(as_, t + b"AG"), (de + 1, t + b"AG" + b"GT")]
    elif aim == "refused-donor":      # the whole donor exon can move behind it
        edits += [(ds, b"GT" + t), (as_ - k - 4, b"AG" + b"GT" + t)]
    return dict(edits=edits, ds=ds, de=de, as_=as_, ae=ae, aim=aim)


def finish_case(rng, gen, c, aimed=None):
    """the EST and the factors of a planted intron over the edited sequence: the two exons joined (with substitutions,
    indels, an unaligned gap, lower case or N near the junction) between 64 bases of padding, the factors the true ones
    with the border moved -> (est, donor, acceptor, first, settings) or None"""
    ds, de, as_, ae = c["ds"], c["de"], c["as_"], c["ae"]
    ex1, ex2 = bytearray(gen[ds:de + 1]), bytearray(gen[as_:ae + 1])
    if c.get("aim") == "attached":                  # the donor's bases continue the acceptor exon to the left
        ex1 = bytearray(gen[as_ - len(ex1):as_])
    r = rng.random()
    near1 = max(0, len(ex1) - 1 - int(rng.integers(0, 12)))
    near2 = min(len(ex2) - 1, int(rng.integers(0, 12)))
    if r < 0.2:
        ex1[near1] = b"ACGT"[int(rng.integers(4))]
    elif r < 0.35:
        ex2[near2] = b"ACGT"[int(rng.integers(4))]
    elif r < 0.42 and len(ex1) > 4:
        del ex1[near1]
    elif r < 0.5:
        ex2.insert(near2, b"ACGT"[int(rng.integers(4))])
    elif r < 0.55:
        ex1[near1] = ord("N")
    elif r < 0.6:
        ex2[near2:near2 + 3] = bytes(ex2[near2:near2 + 3]).lower()
    elif r < 0.66:
        ex1[near1] = b"ACGT"[int(rng.integers(4))]
        ex2[near2] = b"ACGT"[int(rng.integers(4))]
    gap = rnd(rng, int(rng.integers(1, 9))) if rng.random() < 0.12 else b""
    lead, trail = b"A" * 64, b"T" * 64               # the exons lie 64 bases inside the EST; nothing reads the padding
    est = lead + bytes(ex1) + gap + bytes(ex2) + trail
    e1s, e1e = len(lead), len(lead) + len(ex1) - 1
    e2s = e1e + 1 + len(gap)
    e2e = e2s + len(ex2) - 1
    # move the border: the factorization put `m` bases of one exon on the other side (0 - 25)
    m = int(rng.integers(0, 26)) if aimed is None else aimed
    if rng.random() < 0.5:
        m = -m
    donor = [e1s, e1e + m, ds, de + m]
    acceptor = [e2s + m, e2e, as_ + m, ae]
    if gap:
        donor[1], acceptor[0] = e1e + min(m, 0), e2s + max(m, 0)
    if rng.random() < 0.25:                         # the two borders disagree by a little
        donor[3] += int(rng.integers(-3, 4))
    if rng.random() < 0.15:
        acceptor[2] += int(rng.integers(-3, 4))
    if not (donor[0] <= donor[1] < acceptor[0] <= acceptor[1] and donor[2] <= donor[3] < acceptor[2] <= acceptor[3]):
        return None
    first = bool(rng.random() < 0.3)
    if rng.random() < 0.8:
        sp = (30, 70, 30)
    else:
        sp = (int(rng.integers(8, 41)), int(rng.integers(10, 91)), int(rng.integers(8, 41)))
    ilen = acceptor[2] - donor[3] - 1
    mil = (40, 40, 4, 60, ilen, ilen + 2, ilen + 30)[int(rng.integers(7))]
    return est, tuple(donor), tuple(acceptor), first, sp + (mil,)


def query_array(items):
    """items of (est, est_row, gen_row, v, donor, acceptor, first, settings) -> (ests, rows, numpy queries in the
    layout of pgpu_refine_query); equal ESTs and equal row pairs are stored once"""
    q = np.zeros(len(items), dtype=np.dtype(QUERY_DTYPE))
    ests, rows, eat, rat, eoff, roff = [], [], {}, {}, 0, 0
    for i, (est, er, gr, v, donor, acceptor, first, st) in enumerate(items):
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        if (er, gr) not in rat:
            rat[(er, gr)] = roff
            rows += [er, gr]
            roff += 2 * len(gr)
        q[i] = (eat[est], len(est), 1 if first else 0, rat[(er, gr)], len(gr)) + tuple(v) + (tuple(donor), tuple(acceptor)) + tuple(st)
    return b"".join(ests), b"".join(rows), q


_FACTOR = [("EST_start", "<i4"), ("EST_end", "<i4"), ("GEN_start", "<i4"), ("GEN_end", "<i4")]
QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("flags", "<u4"), ("rows_off", "<u8"), ("dim", "<u4"),
               ("factor_cut", "<i4"), ("intron_start", "<i4"), ("intron_end", "<i4"), ("intron_start_on_align", "<i4"),
               ("intron_end_on_align", "<i4"), ("donor", _FACTOR), ("acceptor", _FACTOR),
               ("suffpref_length_on_est", "<i4"), ("suffpref_length_for_intron", "<i4"), ("suffpref_length_on_gen", "<i4"),
               ("min_intron_length", "<i4")]


def result_tuple(r):
    """one element of the result array -> (status, refined, path, donor, acceptor) as refine() gives them"""
    return (int(r["status"]), int(r["refined"]), int(r["path"]), tuple(int(x) for x in r["donor"]), tuple(int(x) for x in r["acceptor"]))


def load_fixture():
    """(genomic bytes, [case dicts: est, donor, acceptor, first, settings, refined, donor_after, acceptor_after, path])"""
    doc = json.load(gzip.open(FIXTURE, "rt"))
    g = bytearray(fixture_genomic())
    assert len(g) == doc["length"]
    for pos, s in doc["edits"]:
        g[pos:pos + len(s)] = s.encode()
    cases = []
    for est, d, a, first, st, refined, d2, a2, path in doc["cases"]:
        cases.append(dict(est=est.encode(), donor=tuple(d), acceptor=tuple(a), first=bool(first), settings=tuple(st),
                          refined=refined, donor_after=tuple(d2), acceptor_after=tuple(a2), path=path))
    return bytes(g), cases
