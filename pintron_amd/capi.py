"""ctypes binding of include/pintron_gpu.h (the C-ABI of libpintron_gpu.so)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpintron_gpu.so")

PGPU_OK, PGPU_EDEVICE, PGPU_ENOMEM, PGPU_EINVAL, PGPU_ENOSPC, PGPU_ERANGE, PGPU_ENOSYS = \
    0, -5, -12, -22, -28, -34, -38
ALIGN, GAP, ED, KBAND, LCF, BORDERS, AFFIX = range(7)
KIND_NAMES = ["ALIGN", "GAP", "ED", "KBAND", "LCF", "BORDERS", "AFFIX"]
JOB_A_GENOMIC, JOB_B_GENOMIC = 1, 2


class DpJob(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("a_off", C.c_uint64),
                ("b_off", C.c_uint64), ("a_len", C.c_uint32), ("b_len", C.c_uint32),
                ("p0", C.c_uint32), ("p1", C.c_uint32), ("p2", C.c_uint32), ("tail", C.c_uint32)]


class DpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("v", C.c_int32 * 6), ("pad", C.c_int32),
                ("str", C.c_uint64 * 2)]


class GroupInfo(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kind", C.c_int32), ("pad", C.c_int32),
                ("jobs", C.c_uint64), ("cells", C.c_uint64), ("algo_bytes", C.c_uint64),
                ("ms", C.c_double), ("t0_ms", C.c_double)]


class PairingParams(C.Structure):
    _fields_ = [("min_factor_len", C.c_uint32), ("reserved", C.c_uint32),
                ("min_string_depth_rate", C.c_double)]


class Pairing(C.Structure):
    _fields_ = [("p", C.c_int32), ("t", C.c_int32), ("l", C.c_int32)]


class FindQuery(C.Structure):       # pgpu_find_query
    _fields_ = [("pat_off", C.c_uint64), ("pat_len", C.c_uint32), ("reserved", C.c_uint32),
                ("lo", C.c_uint32), ("hi", C.c_uint32)]


class Intron(C.Structure):          # pgpu_intron: both ends inclusive
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32)]


class SexonQuery(C.Structure):      # pgpu_sexon_query (36 bytes of fields, padded to 40 by its uint64)
    _fields_ = [("e_off", C.c_uint64), ("elen", C.c_uint32), ("allgstart", C.c_uint32), ("allglen", C.c_uint32),
                ("f1slen", C.c_uint32), ("f2plen", C.c_uint32), ("min_intron_len", C.c_uint32), ("reserved", C.c_uint32)]


class SexonResult(C.Structure):     # pgpu_sexon_result
    _fields_ = [("status", C.c_int32), ("len", C.c_uint32), ("offstart", C.c_uint32), ("offend", C.c_uint32),
                ("gpos", C.c_uint32), ("i1type", C.c_uint32), ("i2type", C.c_uint32), ("pad", C.c_uint32)]


class Factor(C.Structure):         # pgpu_factor: the reference's _factor, all four inclusive
    _fields_ = [("EST_start", C.c_int32), ("EST_end", C.c_int32), ("GEN_start", C.c_int32), ("GEN_end", C.c_int32)]


class RefineQuery(C.Structure):    # pgpu_refine_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("flags", C.c_uint32), ("rows_off", C.c_uint64),
                ("dim", C.c_uint32), ("factor_cut", C.c_int32), ("intron_start", C.c_int32), ("intron_end", C.c_int32),
                ("intron_start_on_align", C.c_int32), ("intron_end_on_align", C.c_int32), ("donor", Factor), ("acceptor", Factor),
                ("suffpref_length_on_est", C.c_int32), ("suffpref_length_for_intron", C.c_int32),
                ("suffpref_length_on_gen", C.c_int32), ("min_intron_length", C.c_int32)]


class RefineResult(C.Structure):   # pgpu_refine_result
    _fields_ = [("status", C.c_int32), ("refined", C.c_int32), ("path", C.c_int32), ("pad", C.c_int32),
                ("donor", Factor), ("acceptor", Factor)]


class ChainQuery(C.Structure):     # pgpu_chain_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("first_exon", C.c_uint32), ("n_exons", C.c_uint32),
                ("reserved", C.c_uint32), ("suffpref_length_on_est", C.c_int32), ("suffpref_length_for_intron", C.c_int32),
                ("suffpref_length_on_gen", C.c_int32), ("min_intron_length", C.c_int32)]


class ChainResult(C.Structure):    # pgpu_chain_result
    _fields_ = [("status", C.c_int32), ("done", C.c_uint32), ("dropped_first", C.c_uint32), ("pad", C.c_uint32)]


class CleanQuery(C.Structure):     # pgpu_clean_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("first_exon", C.c_uint32), ("n_exons", C.c_uint32),
                ("reserved", C.c_uint32), ("complexity_threshold", C.c_double)]


class CleanResult(C.Structure):    # pgpu_clean_result
    _fields_ = [("status", C.c_int32), ("verdict", C.c_uint32), ("first_kept", C.c_uint32), ("n_kept", C.c_uint32)]


class GapsQuery(C.Structure):      # pgpu_gaps_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("first_exon", C.c_uint32), ("n_exons", C.c_uint32),
                ("reserved", C.c_uint32)]


class GapsResult(C.Structure):     # pgpu_gaps_result
    _fields_ = [("status", C.c_int32), ("verdict", C.c_uint32), ("total_edit", C.c_uint32), ("n_kept", C.c_uint32)]


class TailQuery(C.Structure):      # pgpu_tail_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("first_exon", C.c_uint32), ("n_exons", C.c_uint32),
                ("reserved", C.c_uint32), ("orig_off", C.c_uint64)]


class TailResult(C.Structure):     # pgpu_tail_result
    _fields_ = [("status", C.c_int32), ("verdict", C.c_uint8), ("polyA", C.c_uint8), ("polyadenil", C.c_uint8),
                ("recovered", C.c_uint8), ("n_kept", C.c_uint32), ("tail_added", C.c_uint32)]


SmallQuery = TailQuery             # pgpu_small_query: est_off the working sequence, orig_off the original one


class SmallParams(C.Structure):    # pgpu_small_params
    _fields_ = [("min_intron_length", C.c_int32), ("reserved", C.c_uint32)]


class SmallResult(C.Structure):    # pgpu_small_result
    _fields_ = [("status", C.c_int32), ("refused", C.c_uint8), ("verdict", C.c_uint8), ("prefix_added", C.c_uint8),
                ("reserved", C.c_uint8), ("n_added", C.c_uint32), ("n_list", C.c_uint32), ("first_kept", C.c_uint32),
                ("n_kept", C.c_uint32)]


class CandParams(C.Structure):     # pgpu_cand_params
    _fields_ = [("min_factor_len", C.c_uint32), ("min_intron_length", C.c_int32)]


class CandResult(C.Structure):     # pgpu_cand_result
    _fields_ = [("kind", C.c_uint32), ("work", C.c_uint32), ("first_exon", C.c_uint32), ("n_exons", C.c_uint16),
                ("n_pairs", C.c_uint16)]


class EnumResult(C.Structure):     # pgpu_enum_result
    _fields_ = [("kind", C.c_uint16), ("detail", C.c_uint16), ("work", C.c_uint32), ("first_candidate", C.c_uint32),
                ("n_candidates", C.c_uint16), ("n_roots", C.c_uint16)]


class EnumCandidate(C.Structure):  # pgpu_enum_candidate
    _fields_ = [("first_exon", C.c_uint32), ("n_exons", C.c_uint16), ("n_pairs", C.c_uint16), ("root", C.c_uint32),
                ("reserved", C.c_uint32)]


class FactParams(C.Structure):     # pgpu_fact_params
    _fields_ = [("complexity_threshold", C.c_double), ("suffpref_length_on_est", C.c_int32),
                ("suffpref_length_for_intron", C.c_int32), ("suffpref_length_on_gen", C.c_int32), ("min_intron_length", C.c_int32)]


class FactResult(C.Structure):     # pgpu_fact_result
    _fields_ = [("outcome", C.c_uint8), ("stage", C.c_uint8), ("detail", C.c_uint16), ("first_exon", C.c_uint32),
                ("n_exons", C.c_uint16), ("n_merged", C.c_uint16), ("total_edit", C.c_uint32)]


FactQuery = GapsQuery              # pgpu_fact_query: n_exons == 0 is "no candidate"


class FlistParams(C.Structure):    # pgpu_flist_params
    _fields_ = [("complexity_threshold", C.c_double), ("suffpref_length_on_est", C.c_int32),
                ("suffpref_length_for_intron", C.c_int32), ("suffpref_length_on_gen", C.c_int32), ("min_intron_length", C.c_int32),
                ("max_coverage_diff", C.c_double), ("max_site_difference", C.c_int32), ("max_gaplength_diff", C.c_int32),
                ("max_number_of_factorizations", C.c_int32), ("reserved", C.c_uint32)]


class FlistQuery(C.Structure):     # pgpu_flist_query
    _fields_ = [("est_off", C.c_uint64), ("est_len", C.c_uint32), ("first_candidate", C.c_uint32), ("n_candidates", C.c_uint32),
                ("reserved", C.c_uint32)]


class FlistResult(C.Structure):    # pgpu_flist_result
    _fields_ = [("outcome", C.c_uint8), ("stage", C.c_uint8), ("detail", C.c_uint16), ("first_fact", C.c_uint32),
                ("n_facts", C.c_uint16), ("n_cleaned", C.c_uint16), ("n_listed", C.c_uint16), ("n_filtered", C.c_uint16)]


class FlistFact(C.Structure):      # pgpu_flist_fact
    _fields_ = [("first_exon", C.c_uint32), ("n_exons", C.c_uint16), ("n_merged", C.c_uint16), ("candidate", C.c_uint32),
                ("total_edit", C.c_uint16), ("flags", C.c_uint16)]


class FinalResult(C.Structure):    # pgpu_final_result
    _fields_ = [("outcome", C.c_uint8), ("stage", C.c_uint8), ("detail", C.c_uint16), ("first_exon", C.c_uint32),
                ("n_exons", C.c_uint16), ("n_merged", C.c_uint16), ("total_edit", C.c_uint32), ("tail_added", C.c_uint32),
                ("polyA", C.c_uint8), ("polyadenil", C.c_uint8), ("recovered", C.c_uint8), ("refused", C.c_uint8),
                ("n_removed", C.c_uint16), ("n_added", C.c_uint16), ("n_cleaned", C.c_uint16), ("prefix_added", C.c_uint8),
                ("reserved", C.c_uint8)]


FinalQuery = TailQuery             # pgpu_final_query: n_exons == 0 is "no candidate"


class UnitQuery(C.Structure):      # pgpu_unit_query
    _fields_ = [("est_index", C.c_uint32), ("fwd", C.c_uint32), ("rev", C.c_uint32), ("flags", C.c_uint32)]


class UnitParams(C.Structure):     # pgpu_unit_params
    _fields_ = [("pref_N_length", C.c_int32), ("retain_externals", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class UnitResult(C.Structure):     # pgpu_unit_result
    _fields_ = [("verdict", C.c_uint8), ("strand", C.c_uint8), ("reason", C.c_uint8), ("n_factorizations", C.c_uint8),
                ("pattern", C.c_uint32), ("first_byte", C.c_uint64), ("n_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class TextResult(C.Structure):     # pgpu_text_result
    _fields_ = [("raw_first", C.c_uint64), ("pests_first", C.c_uint64), ("raw_bytes", C.c_uint32), ("pests_bytes", C.c_uint32),
                ("verdict", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class SideResult(C.Structure):     # pgpu_side_result
    _fields_ = [("megs_first", C.c_uint64), ("pmegs_first", C.c_uint64), ("edges_first", C.c_uint64), ("megs_bytes", C.c_uint32),
                ("pmegs_bytes", C.c_uint32), ("edges_bytes", C.c_uint32), ("verdict", C.c_uint8), ("reserved", C.c_uint8 * 3)]


REFINE_MAX_DIM, REFINE_MAX_ED, REFINE_FIRST_INTRON = 1024, 256, 1
CHAIN_MAX_EST_WINDOW, CHAIN_MAX_GEN_WINDOW = 192, 320
_FACTOR_DTYPE = [("EST_start", "<i4"), ("EST_end", "<i4"), ("GEN_start", "<i4"), ("GEN_end", "<i4")]
REFINE_QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("flags", "<u4"), ("rows_off", "<u8"), ("dim", "<u4"),
                      ("factor_cut", "<i4"), ("intron_start", "<i4"), ("intron_end", "<i4"), ("intron_start_on_align", "<i4"),
                      ("intron_end_on_align", "<i4"), ("donor", _FACTOR_DTYPE), ("acceptor", _FACTOR_DTYPE),
                      ("suffpref_length_on_est", "<i4"), ("suffpref_length_for_intron", "<i4"), ("suffpref_length_on_gen", "<i4"),
                      ("min_intron_length", "<i4")]
REFINE_RESULT_DTYPE = [("status", "<i4"), ("refined", "<i4"), ("path", "<i4"), ("pad", "<i4"), ("donor", _FACTOR_DTYPE),
                       ("acceptor", _FACTOR_DTYPE)]

CHAIN_QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("first_exon", "<u4"), ("n_exons", "<u4"), ("reserved", "<u4"),
                     ("suffpref_length_on_est", "<i4"), ("suffpref_length_for_intron", "<i4"), ("suffpref_length_on_gen", "<i4"),
                     ("min_intron_length", "<i4")]
CHAIN_RESULT_DTYPE = [("status", "<i4"), ("done", "<u4"), ("dropped_first", "<u4"), ("pad", "<u4")]
FACTOR_DTYPE = _FACTOR_DTYPE
CLEAN_MAX_EXONS, CLEAN_MAX_END_EXON = 64, 4096
CLEAN_QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("first_exon", "<u4"), ("n_exons", "<u4"), ("reserved", "<u4"),
                     ("complexity_threshold", "<f8")]
CLEAN_RESULT_DTYPE = [("status", "<i4"), ("verdict", "<u4"), ("first_kept", "<u4"), ("n_kept", "<u4")]
GAPS_MAX_EXONS, GAPS_MAX_EST_GAP, GAPS_MAX_ERRORS = 64, 64, 20
GAPS_QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("first_exon", "<u4"), ("n_exons", "<u4"), ("reserved", "<u4")]
GAPS_RESULT_DTYPE = [("status", "<i4"), ("verdict", "<u4"), ("total_edit", "<u4"), ("n_kept", "<u4")]
TAIL_MAX_EXONS, TAIL_MAX_AFFIX, TAIL_MAX_SMALL_WINDOW, TAIL_MAX_SMALL_GEN = 64, 256, 128, 256
TAIL_UB_MED_EXON, TAIL_AFFIXES_LENGTH = 100, 5
TAIL_QUERY_DTYPE = GAPS_QUERY_DTYPE + [("orig_off", "<u8")]
TAIL_RESULT_DTYPE = [("status", "<i4"), ("verdict", "u1"), ("polyA", "u1"), ("polyadenil", "u1"), ("recovered", "u1"),
                     ("n_kept", "<u4"), ("tail_added", "<u4")]
SMALL_MAX_EXONS, SMALL_MAX_PREFIX_WINDOW, SMALL_MAX_KBAND = 64, 256, 31
SMALL_QUERY_DTYPE = TAIL_QUERY_DTYPE
SMALL_PARAMS_DTYPE = [("min_intron_length", "<i4"), ("reserved", "<u4")]
SMALL_RESULT_DTYPE = [("status", "<i4"), ("refused", "u1"), ("verdict", "u1"), ("prefix_added", "u1"), ("reserved", "u1"),
                      ("n_added", "<u4"), ("n_list", "<u4"), ("first_kept", "<u4"), ("n_kept", "<u4")]
CAND_NONE, CAND_NOT_PATH, CAND_REFUSED, CAND_ONE = range(4)
MEG_TOO_COMPLEX, MEG_UNAVAILABLE = 1, 2
ENUM_NONE, ENUM_CYCLIC, ENUM_RANGE, ENUM_LISTS = range(4)
ENUM_CAP_LIST, ENUM_CAP_EMBEDDINGS = 1, 2
ENUM_MAX_LIST, ENUM_MAX_EMBEDDINGS = 64, 512
ENUM_RESULT_DTYPE = [("kind", "<u2"), ("detail", "<u2"), ("work", "<u4"), ("first_candidate", "<u4"), ("n_candidates", "<u2"),
                     ("n_roots", "<u2")]
ENUM_CANDIDATE_DTYPE = [("first_exon", "<u4"), ("n_exons", "<u2"), ("n_pairs", "<u2"), ("root", "<u4"), ("reserved", "<u4")]
CAND_PARAMS_DTYPE = [("min_factor_len", "<u4"), ("min_intron_length", "<i4")]
CAND_RESULT_DTYPE = [("kind", "<u4"), ("work", "<u4"), ("first_exon", "<u4"), ("n_exons", "<u2"), ("n_pairs", "<u2")]
FACT_HOST, FACT_EMPTY, FACT_DONE = range(3)
FACT_PARAMS_DTYPE = [("complexity_threshold", "<f8"), ("suffpref_length_on_est", "<i4"), ("suffpref_length_for_intron", "<i4"),
                     ("suffpref_length_on_gen", "<i4"), ("min_intron_length", "<i4")]
FACT_RESULT_DTYPE = [("outcome", "u1"), ("stage", "u1"), ("detail", "<u2"), ("first_exon", "<u4"), ("n_exons", "<u2"),
                     ("n_merged", "<u2"), ("total_edit", "<u4")]
FACT_QUERY_DTYPE = GAPS_QUERY_DTYPE
FLIST_MAX_CANDIDATES, FLIST_CAP_CANDIDATES = 64, 4
FLIST_DROPPED_FIRST, FLIST_HEAD_WIDENED, FLIST_TAIL_WIDENED = 1, 2, 4
FLIST_PARAMS_DTYPE = FACT_PARAMS_DTYPE + [("max_coverage_diff", "<f8"), ("max_site_difference", "<i4"), ("max_gaplength_diff", "<i4"),
                                          ("max_number_of_factorizations", "<i4"), ("reserved", "<u4")]
FLIST_QUERY_DTYPE = [("est_off", "<u8"), ("est_len", "<u4"), ("first_candidate", "<u4"), ("n_candidates", "<u4"), ("reserved", "<u4")]
FLIST_RESULT_DTYPE = [("outcome", "u1"), ("stage", "u1"), ("detail", "<u2"), ("first_fact", "<u4"), ("n_facts", "<u2"),
                      ("n_cleaned", "<u2"), ("n_listed", "<u2"), ("n_filtered", "<u2")]
FLIST_FACT_DTYPE = [("first_exon", "<u4"), ("n_exons", "<u2"), ("n_merged", "<u2"), ("candidate", "<u4"), ("total_edit", "<u2"),
                    ("flags", "<u2")]
FINAL_RESULT_DTYPE = [("outcome", "u1"), ("stage", "u1"), ("detail", "<u2"), ("first_exon", "<u4"), ("n_exons", "<u2"),
                      ("n_merged", "<u2"), ("total_edit", "<u4"), ("tail_added", "<u4"), ("polyA", "u1"), ("polyadenil", "u1"),
                      ("recovered", "u1"), ("refused", "u1"), ("n_removed", "<u2"), ("n_added", "<u2"), ("n_cleaned", "<u2"),
                      ("prefix_added", "u1"), ("reserved", "u1")]
FINAL_QUERY_DTYPE = TAIL_QUERY_DTYPE
UNIT_NO_SIBLING, UNIT_FWD_SUFF_POLYA, UNIT_REV_SUFF_POLYA = 0xffffffff, 1, 2
UNIT_HOST, UNIT_UNALIGNED, UNIT_ALIGNED = range(3)
TEXT_NONE, TEXT_DONE, TEXT_HOST = range(3)
TEXT_MAX_UNIT_BYTES = 1 << 24
TEXT_RESULT_DTYPE = [("raw_first", "<u8"), ("pests_first", "<u8"), ("raw_bytes", "<u4"), ("pests_bytes", "<u4"), ("verdict", "u1"),
                     ("reserved", "u1", (7,))]
SIDE_NONE, SIDE_DONE, SIDE_HOST = range(3)
SIDE_MAX_UNIT_BYTES = 1 << 24
SIDE_RESULT_DTYPE = [("megs_first", "<u8"), ("pmegs_first", "<u8"), ("edges_first", "<u8"), ("megs_bytes", "<u4"), ("pmegs_bytes", "<u4"),
                     ("edges_bytes", "<u4"), ("verdict", "u1"), ("reserved", "u1", (3,))]
UNIT_QUERY_DTYPE = [("est_index", "<u4"), ("fwd", "<u4"), ("rev", "<u4"), ("flags", "<u4")]
UNIT_RESULT_DTYPE = [("verdict", "u1"), ("strand", "u1"), ("reason", "u1"), ("n_factorizations", "u1"), ("pattern", "<u4"),
                     ("first_byte", "<u8"), ("n_bytes", "<u4"), ("reserved", "<u4")]

SEXON_MAX_ELEN = 64
SEXON_QUERY_DTYPE = [("e_off", "<u8"), ("elen", "<u4"), ("allgstart", "<u4"), ("allglen", "<u4"), ("f1slen", "<u4"),
                     ("f2plen", "<u4"), ("min_intron_len", "<u4"), ("reserved", "<u4"), ("_pad", "<u4")]
SEXON_RESULT_DTYPE = [("status", "<i4"), ("len", "<u4"), ("offstart", "<u4"), ("offend", "<u4"), ("gpos", "<u4"),
                      ("i1type", "<u4"), ("i2type", "<u4"), ("pad", "<u4")]

assert C.sizeof(DpJob) == 48 and C.sizeof(DpResult) == 48 and C.sizeof(FindQuery) == 24
assert C.sizeof(Intron) == 8 and C.sizeof(SexonQuery) == 40 and C.sizeof(SexonResult) == 32
assert C.sizeof(Factor) == 16 and C.sizeof(RefineQuery) == 96 and C.sizeof(RefineResult) == 48
assert C.sizeof(ChainQuery) == 40 and C.sizeof(ChainResult) == 16
assert C.sizeof(CleanQuery) == 32 and C.sizeof(CleanResult) == 16
assert C.sizeof(GapsQuery) == 24 and C.sizeof(GapsResult) == 16
assert C.sizeof(TailQuery) == 32 and C.sizeof(TailResult) == 16
assert C.sizeof(SmallParams) == 8 and C.sizeof(SmallResult) == 24
assert C.sizeof(CandParams) == 8 and C.sizeof(CandResult) == 16
assert C.sizeof(FactParams) == 24 and C.sizeof(FactResult) == 16
assert C.sizeof(FinalResult) == 32 and C.sizeof(FinalQuery) == 32
assert C.sizeof(FlistParams) == 48 and C.sizeof(FlistQuery) == 24 and C.sizeof(FlistResult) == 16 and C.sizeof(FlistFact) == 16
assert C.sizeof(UnitQuery) == 16 and C.sizeof(UnitParams) == 8 and C.sizeof(UnitResult) == 24
assert C.sizeof(TextResult) == 32
assert C.sizeof(SideResult) == 40

# every symbol include/pintron_gpu.h declares
EXPORTS = [
    "pgpu_init", "pgpu_destroy", "pgpu_last_error", "pgpu_abi_version", "pgpu_set_timing", "pgpu_device_numa_node",
    "pgpu_index_build", "pgpu_index_destroy", "pgpu_index_suffix_array", "pgpu_index_save", "pgpu_index_load", "pgpu_pairings",
    "pgpu_index_find", "pgpu_index_find_kernel_ms",
    "pgpu_index_classify", "pgpu_index_score5", "pgpu_index_small_exons", "pgpu_index_small_exons_kernel_ms",
    "pgpu_index_refine_introns", "pgpu_index_refine_introns_kernel_ms",
    "pgpu_index_refine_chains", "pgpu_index_refine_chains_kernel_ms",
    "pgpu_index_clean_chains", "pgpu_index_clean_chains_kernel_ms",
    "pgpu_index_gap_chains", "pgpu_index_gap_chains_kernel_ms",
    "pgpu_index_tail_chains", "pgpu_index_tail_chains_kernel_ms",
    "pgpu_index_small_chains", "pgpu_index_small_chains_kernel_ms",
    "pgpu_index_tail_chains_wide", "pgpu_index_small_chains_wide",
    "pgpu_index_final_factorizations_wide", "pgpu_pairing_plan_run_final_factorizations_wide",
    "pgpu_pairing_plan_create", "pgpu_pairing_plan_create_resident", "pgpu_pairing_plan_run", "pgpu_pairing_plan_count",
    "pgpu_pairing_plan_positions", "pgpu_pairing_plan_kernel_ms", "pgpu_pairing_plan_fetch",
    "pgpu_pairing_plan_destroy",
    "pgpu_pairing_plan_run_meg", "pgpu_pairing_plan_meg_bytes", "pgpu_pairing_plan_fetch_meg",
    "pgpu_pairing_plan_meg_ms", "pgpu_host_alloc", "pgpu_host_free",
    "pgpu_pairing_plan_run_candidates", "pgpu_pairing_plan_candidate_exons", "pgpu_pairing_plan_fetch_candidates",
    "pgpu_pairing_plan_candidates_ms", "pgpu_index_candidates", "pgpu_index_candidates_kernel_ms",
    "pgpu_pairing_plan_run_candidate_lists", "pgpu_pairing_plan_candidate_list_counts", "pgpu_pairing_plan_fetch_candidate_lists",
    "pgpu_pairing_plan_candidate_lists_ms", "pgpu_index_candidate_lists", "pgpu_index_candidate_lists_kernel_ms",
    "pgpu_pairing_plan_run_factorizations", "pgpu_pairing_plan_factorization_exons", "pgpu_pairing_plan_fetch_factorizations",
    "pgpu_pairing_plan_factorizations_ms", "pgpu_index_factorizations", "pgpu_index_factorizations_kernel_ms",
    "pgpu_index_factorization_lists", "pgpu_index_factorization_lists_kernel_ms", "pgpu_pairing_plan_run_factorization_lists",
    "pgpu_pairing_plan_factorization_list_counts", "pgpu_pairing_plan_fetch_factorization_lists",
    "pgpu_pairing_plan_factorization_lists_ms",
    "pgpu_pairing_plan_create_with_originals", "pgpu_pairing_plan_run_final_factorizations", "pgpu_pairing_plan_final_exons",
    "pgpu_pairing_plan_fetch_final_factorizations", "pgpu_pairing_plan_final_ms", "pgpu_index_final_factorizations",
    "pgpu_index_final_factorizations_kernel_ms",
    "pgpu_unit_records", "pgpu_unit_records_kernel_ms", "pgpu_pairing_plan_run_units", "pgpu_pairing_plan_unit_bytes",
    "pgpu_pairing_plan_fetch_units", "pgpu_pairing_plan_units_ms",
    "pgpu_text_source_create", "pgpu_text_source_destroy", "pgpu_unit_texts", "pgpu_unit_texts_kernel_ms",
    "pgpu_pairing_plan_run_texts", "pgpu_pairing_plan_text_bytes", "pgpu_pairing_plan_fetch_texts", "pgpu_pairing_plan_texts_ms",
    "pgpu_pairing_plan_texts_write_ms",
    "pgpu_unit_sides", "pgpu_unit_sides_kernel_ms", "pgpu_pairing_plan_run_sides", "pgpu_pairing_plan_side_bytes",
    "pgpu_pairing_plan_fetch_sides", "pgpu_pairing_plan_sides_ms", "pgpu_pairing_plan_sides_write_ms",
    "pgpu_comm_unique_id", "pgpu_comm_init", "pgpu_gather", "pgpu_allgather", "pgpu_comm_destroy",
    "pgpu_range_push", "pgpu_range_pop", "pgpu_build_info",
    "pgpu_dp_plan_create", "pgpu_dp_plan_create_parts", "pgpu_dp_plan_launch", "pgpu_dp_plan_sync",
    "pgpu_dp_plan_string_bytes", "pgpu_dp_plan_fetch", "pgpu_dp_plan_destroy",
    "pgpu_dp_plan_results_to_device",
    "pgpu_dp_plan_cells", "pgpu_dp_plan_algo_bytes", "pgpu_dp_plan_kernel_ms",
    "pgpu_dp_plan_launches", "pgpu_dp_plan_n_groups", "pgpu_dp_plan_group_info", "pgpu_dp_batch",
]

_lib = None


class PgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pgpu error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load libpintron_gpu.so (no fallback: a missing library is an error)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, u64, sz = C.c_void_p, C.c_uint64, C.c_size_t
        L.pgpu_init.argtypes = [C.c_int, C.POINTER(vp)]
        L.pgpu_destroy.argtypes = [vp]
        L.pgpu_set_timing.argtypes = [vp, C.c_int]
        L.pgpu_last_error.argtypes = [vp]
        L.pgpu_last_error.restype = C.c_char_p
        L.pgpu_build_info.restype = C.c_char_p
        L.pgpu_range_push.argtypes = [C.c_char_p]
        L.pgpu_range_push.restype = None
        L.pgpu_range_pop.restype = None
        L.pgpu_allgather.argtypes = [vp, vp, vp, u64, vp]
        L.pgpu_index_build.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp)]
        L.pgpu_index_destroy.argtypes = [vp, vp]
        L.pgpu_index_save.argtypes = [vp, vp, C.c_char_p, C.c_char_p]
        L.pgpu_index_load.argtypes = [vp, C.c_char_p, C.c_char_p, sz, C.POINTER(vp)]
        L.pgpu_index_suffix_array.argtypes = [vp, vp, C.POINTER(C.c_uint32), sz]
        L.pgpu_index_find.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(FindQuery), sz,
                                      C.POINTER(C.c_uint32), sz, C.POINTER(u64), C.POINTER(sz)]
        L.pgpu_index_find_kernel_ms.argtypes = [C.c_int]
        L.pgpu_index_find_kernel_ms.restype = C.c_double
        L.pgpu_index_classify.argtypes = [vp, vp, C.POINTER(Intron), sz, C.POINTER(C.c_uint8)]
        L.pgpu_index_score5.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_double), sz]
        L.pgpu_index_small_exons.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(SexonQuery), sz, C.POINTER(SexonResult)]
        L.pgpu_index_small_exons_kernel_ms.argtypes = []
        L.pgpu_index_small_exons_kernel_ms.restype = C.c_double
        L.pgpu_index_refine_introns.argtypes = [vp, vp, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(RefineQuery), sz,
                                                C.POINTER(RefineResult)]
        L.pgpu_index_refine_introns_kernel_ms.argtypes = []
        L.pgpu_index_refine_introns_kernel_ms.restype = C.c_double
        L.pgpu_index_refine_chains.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(ChainQuery), sz,
                                               C.POINTER(Factor), C.POINTER(C.c_uint8), C.POINTER(ChainResult)]
        L.pgpu_index_refine_chains_kernel_ms.argtypes = []
        L.pgpu_index_refine_chains_kernel_ms.restype = C.c_double
        L.pgpu_index_clean_chains.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(CleanQuery), sz,
                                              C.POINTER(Factor), C.POINTER(C.c_uint8), C.POINTER(CleanResult)]
        L.pgpu_index_clean_chains_kernel_ms.argtypes = []
        L.pgpu_index_clean_chains_kernel_ms.restype = C.c_double
        L.pgpu_index_gap_chains.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(GapsQuery), sz,
                                            C.POINTER(Factor), C.POINTER(C.c_uint8), C.POINTER(GapsResult)]
        L.pgpu_index_gap_chains_kernel_ms.argtypes = []
        L.pgpu_index_gap_chains_kernel_ms.restype = C.c_double
        L.pgpu_index_tail_chains.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(TailQuery), sz,
                                             C.POINTER(Factor), C.POINTER(C.c_uint8), C.POINTER(TailResult)]
        L.pgpu_index_tail_chains_wide.argtypes = L.pgpu_index_tail_chains.argtypes
        L.pgpu_index_tail_chains_kernel_ms.argtypes = []
        L.pgpu_index_tail_chains_kernel_ms.restype = C.c_double
        L.pgpu_index_small_chains.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(SmallQuery), sz,
                                              C.POINTER(SmallParams), C.POINTER(Factor), C.POINTER(C.c_uint8),
                                              C.POINTER(SmallResult)]
        L.pgpu_index_small_chains_wide.argtypes = L.pgpu_index_small_chains.argtypes
        L.pgpu_index_small_chains_kernel_ms.argtypes = []
        L.pgpu_index_small_chains_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_meg.argtypes = [vp, vp, vp]
        L.pgpu_pairing_plan_meg_bytes.argtypes = [vp]
        L.pgpu_pairing_plan_meg_bytes.restype = u64
        L.pgpu_pairing_plan_meg_ms.argtypes = [vp]
        L.pgpu_pairing_plan_meg_ms.restype = C.c_double
        L.pgpu_pairing_plan_fetch_meg.argtypes = [vp, vp, vp, sz, C.POINTER(u64)]
        L.pgpu_pairing_plan_run_candidates.argtypes = [vp, vp, C.POINTER(CandParams)]
        L.pgpu_pairing_plan_candidate_exons.argtypes = [vp]
        L.pgpu_pairing_plan_candidate_exons.restype = u64
        L.pgpu_pairing_plan_fetch_candidates.argtypes = [vp, vp, C.POINTER(CandResult), C.POINTER(Factor), sz]
        L.pgpu_pairing_plan_candidates_ms.argtypes = [vp]
        L.pgpu_pairing_plan_candidates_ms.restype = C.c_double
        L.pgpu_index_candidates.argtypes = [vp, vp, vp, sz, C.POINTER(u64), sz, C.POINTER(CandParams), C.POINTER(CandResult),
                                            C.POINTER(Factor), sz, C.POINTER(sz)]
        L.pgpu_index_candidates_kernel_ms.argtypes = []
        L.pgpu_index_candidates_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_candidate_lists.argtypes = [vp, vp, C.POINTER(CandParams)]
        L.pgpu_pairing_plan_candidate_list_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.pgpu_pairing_plan_fetch_candidate_lists.argtypes = [vp, vp, C.POINTER(EnumResult), C.POINTER(EnumCandidate), sz,
                                                              C.POINTER(Factor), sz]
        L.pgpu_pairing_plan_candidate_lists_ms.argtypes = [vp]
        L.pgpu_pairing_plan_candidate_lists_ms.restype = C.c_double
        L.pgpu_index_candidate_lists.argtypes = [vp, vp, vp, sz, C.POINTER(u64), sz, C.POINTER(CandParams), C.POINTER(EnumResult),
                                                 C.POINTER(EnumCandidate), sz, C.POINTER(Factor), sz, C.POINTER(sz), C.POINTER(sz)]
        L.pgpu_index_candidate_lists_kernel_ms.argtypes = []
        L.pgpu_index_candidate_lists_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_factorizations.argtypes = [vp, vp, C.POINTER(FactParams)]
        L.pgpu_pairing_plan_factorization_exons.argtypes = [vp]
        L.pgpu_pairing_plan_factorization_exons.restype = u64
        L.pgpu_pairing_plan_fetch_factorizations.argtypes = [vp, vp, C.POINTER(FactResult), C.POINTER(Factor),
                                                             C.POINTER(C.c_uint8), sz]
        L.pgpu_pairing_plan_factorizations_ms.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_factorizations_ms.restype = C.c_double
        L.pgpu_index_factorizations.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(FactQuery), sz,
                                                C.POINTER(FactParams), C.POINTER(FactResult), C.POINTER(Factor),
                                                C.POINTER(C.c_uint8), sz, C.POINTER(sz)]
        L.pgpu_index_factorizations_kernel_ms.argtypes = []
        L.pgpu_index_factorizations_kernel_ms.restype = C.c_double
        L.pgpu_index_factorization_lists.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(EnumCandidate), sz, C.POINTER(Factor), sz,
                                                     C.POINTER(FlistQuery), sz, C.POINTER(FlistParams), C.POINTER(FlistResult),
                                                     C.POINTER(FlistFact), sz, C.POINTER(Factor), C.POINTER(C.c_uint8), sz,
                                                     C.POINTER(sz), C.POINTER(sz)]
        L.pgpu_index_factorization_lists_kernel_ms.argtypes = []
        L.pgpu_index_factorization_lists_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_factorization_lists.argtypes = [vp, vp, C.POINTER(FlistParams)]
        L.pgpu_pairing_plan_factorization_list_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.pgpu_pairing_plan_fetch_factorization_lists.argtypes = [vp, vp, C.POINTER(FlistResult), C.POINTER(FlistFact), sz,
                                                                  C.POINTER(Factor), C.POINTER(C.c_uint8), sz]
        L.pgpu_pairing_plan_factorization_lists_ms.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_factorization_lists_ms.restype = C.c_double
        L.pgpu_pairing_plan_create_with_originals.argtypes = [vp, vp, C.c_char_p, C.POINTER(u64), sz, C.c_int,
                                                              C.POINTER(C.c_uint32), C.POINTER(u64), C.c_char_p, sz, C.POINTER(vp)]
        L.pgpu_pairing_plan_run_final_factorizations.argtypes = [vp, vp, C.POINTER(SmallParams)]
        L.pgpu_pairing_plan_run_final_factorizations_wide.argtypes = [vp, vp, C.POINTER(SmallParams)]
        L.pgpu_pairing_plan_final_exons.argtypes = [vp]
        L.pgpu_pairing_plan_final_exons.restype = u64
        L.pgpu_pairing_plan_fetch_final_factorizations.argtypes = [vp, vp, C.POINTER(FinalResult), C.POINTER(Factor),
                                                                   C.POINTER(C.c_uint8), sz]
        L.pgpu_pairing_plan_final_ms.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_final_ms.restype = C.c_double
        L.pgpu_index_final_factorizations.argtypes = [vp, vp, C.c_char_p, sz, C.POINTER(Factor), sz, C.POINTER(FinalQuery), sz,
                                                      C.POINTER(FactParams), C.POINTER(SmallParams), C.POINTER(FinalResult),
                                                      C.POINTER(Factor), C.POINTER(C.c_uint8), sz, C.POINTER(sz)]
        L.pgpu_index_final_factorizations_wide.argtypes = L.pgpu_index_final_factorizations.argtypes
        L.pgpu_index_final_factorizations_kernel_ms.argtypes = []
        L.pgpu_index_final_factorizations_kernel_ms.restype = C.c_double
        L.pgpu_unit_records.argtypes = [vp, C.POINTER(FinalResult), sz, C.POINTER(Factor), sz, C.POINTER(C.c_uint8),
                                        C.POINTER(UnitQuery), sz, C.POINTER(UnitParams), C.POINTER(UnitResult), vp, sz,
                                        C.POINTER(sz)]
        L.pgpu_unit_records_kernel_ms.argtypes = []
        L.pgpu_unit_records_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_units.argtypes = [vp, vp, C.POINTER(UnitQuery), sz, C.POINTER(UnitParams)]
        L.pgpu_pairing_plan_unit_bytes.argtypes = [vp]
        L.pgpu_pairing_plan_unit_bytes.restype = u64
        L.pgpu_pairing_plan_fetch_units.argtypes = [vp, vp, C.POINTER(UnitResult), vp, sz]
        L.pgpu_pairing_plan_units_ms.argtypes = [vp]
        L.pgpu_pairing_plan_units_ms.restype = C.c_double
        L.pgpu_text_source_create.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp)]
        L.pgpu_text_source_destroy.argtypes = [vp, vp]
        L.pgpu_unit_texts.argtypes = [vp, C.POINTER(UnitResult), sz, vp, sz, vp, sz, C.POINTER(u64), vp, sz, C.POINTER(u64), sz,
                                      vp, sz, C.POINTER(TextResult), vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
        L.pgpu_unit_texts_kernel_ms.argtypes = []
        L.pgpu_unit_texts_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_texts.argtypes = [vp, vp, vp, vp, sz, C.POINTER(u64)]
        L.pgpu_pairing_plan_text_bytes.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_text_bytes.restype = u64
        L.pgpu_pairing_plan_fetch_texts.argtypes = [vp, vp, C.POINTER(TextResult), vp, sz, vp, sz]
        L.pgpu_pairing_plan_texts_ms.argtypes = [vp]
        L.pgpu_pairing_plan_texts_ms.restype = C.c_double
        L.pgpu_pairing_plan_texts_write_ms.argtypes = [vp]
        L.pgpu_pairing_plan_texts_write_ms.restype = C.c_double
        L.pgpu_unit_sides.argtypes = [vp, C.POINTER(UnitQuery), C.POINTER(UnitResult), sz, vp, sz, C.POINTER(u64), sz, vp, sz,
                                      C.POINTER(u64), vp, sz, C.POINTER(u64), C.POINTER(SideResult), vp, sz, vp, sz, vp, sz,
                                      C.POINTER(sz)]
        L.pgpu_unit_sides_kernel_ms.argtypes = []
        L.pgpu_unit_sides_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_run_sides.argtypes = [vp, vp]
        L.pgpu_pairing_plan_side_bytes.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_side_bytes.restype = u64
        L.pgpu_pairing_plan_fetch_sides.argtypes = [vp, vp, C.POINTER(SideResult), vp, sz, vp, sz, vp, sz]
        L.pgpu_pairing_plan_sides_ms.argtypes = [vp]
        L.pgpu_pairing_plan_sides_ms.restype = C.c_double
        L.pgpu_pairing_plan_sides_write_ms.argtypes = [vp]
        L.pgpu_pairing_plan_sides_write_ms.restype = C.c_double
        L.pgpu_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
        L.pgpu_host_free.argtypes = [vp, vp]
        L.pgpu_comm_unique_id.argtypes = [vp, vp]
        L.pgpu_comm_init.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.pgpu_gather.argtypes = [vp, vp, C.c_char_p, u64, vp, u64, C.POINTER(u64)]
        L.pgpu_comm_destroy.argtypes = [vp, vp]
        L.pgpu_pairings.argtypes = [vp, vp, C.c_char_p, C.POINTER(u64), sz,
                                    C.POINTER(PairingParams), C.POINTER(Pairing), sz,
                                    C.POINTER(u64), C.POINTER(sz)]
        L.pgpu_pairing_plan_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(u64), sz, C.POINTER(vp)]
        L.pgpu_pairing_plan_create_resident.argtypes = [vp, vp, C.c_char_p, C.POINTER(u64), sz, C.POINTER(vp)]
        L.pgpu_pairing_plan_run.argtypes = [vp, vp, C.POINTER(PairingParams)]
        L.pgpu_pairing_plan_count.argtypes = [vp]
        L.pgpu_pairing_plan_count.restype = u64
        L.pgpu_pairing_plan_positions.argtypes = [vp]
        L.pgpu_pairing_plan_positions.restype = u64
        L.pgpu_pairing_plan_kernel_ms.argtypes = [vp, C.c_int]
        L.pgpu_pairing_plan_kernel_ms.restype = C.c_double
        L.pgpu_pairing_plan_fetch.argtypes = [vp, vp, C.POINTER(Pairing), sz, C.POINTER(u64)]
        L.pgpu_pairing_plan_destroy.argtypes = [vp, vp]
        L.pgpu_dp_plan_create_parts.argtypes = [vp, vp, vp, sz, C.POINTER(vp)]
        L.pgpu_dp_plan_create.argtypes = [vp, vp, C.POINTER(DpJob), sz, C.c_char_p, sz,
                                          C.POINTER(vp)]
        L.pgpu_dp_plan_launch.argtypes = [vp, vp]
        L.pgpu_dp_plan_sync.argtypes = [vp, vp]
        L.pgpu_dp_plan_string_bytes.argtypes = [vp]
        L.pgpu_dp_plan_string_bytes.restype = sz
        L.pgpu_dp_plan_fetch.argtypes = [vp, vp, C.POINTER(DpResult), C.c_char_p, sz]
        L.pgpu_dp_plan_destroy.argtypes = [vp, vp]
        L.pgpu_dp_plan_results_to_device.argtypes = [vp, vp, vp, sz]
        for nm in ("pgpu_dp_plan_cells", "pgpu_dp_plan_algo_bytes", "pgpu_dp_plan_launches"):
            getattr(L, nm).argtypes = [vp, C.c_int]
            getattr(L, nm).restype = u64
        L.pgpu_dp_plan_kernel_ms.argtypes = [vp, C.c_int]
        L.pgpu_dp_plan_kernel_ms.restype = C.c_double
        L.pgpu_dp_plan_n_groups.argtypes = [vp]
        L.pgpu_dp_plan_group_info.argtypes = [vp, C.c_int, C.POINTER(GroupInfo)]
        L.pgpu_dp_batch.argtypes = [vp, vp, C.POINTER(DpJob), sz, C.c_char_p, sz,
                                    C.POINTER(DpResult), C.c_char_p, sz, C.POINTER(sz)]
        _lib = L
    return _lib


class Context:
    """One pgpu_ctx (one HIP stream on one device)."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.pgpu_init(device, C.byref(self.h))
        if rc != PGPU_OK:
            raise PgpuError(rc, "pgpu_init(%d) failed (no usable gfx950 device?)" % device)
        self.L.pgpu_set_timing(self.h, 1)      # tests and bench read the per-kernel timings

    def check(self, rc):
        if rc != PGPU_OK:
            raise PgpuError(rc, self.L.pgpu_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.pgpu_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Index:
    def __init__(self, ctx: Context, genomic: bytes, load_from=None):
        """Built on the device, or (load_from=<path>) read from a file written by save()."""
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n = len(genomic)
        self.genomic = genomic
        if load_from is None:
            ctx.check(ctx.L.pgpu_index_build(ctx.h, genomic, len(genomic), C.byref(self.h)))
        else:
            rc = ctx.L.pgpu_index_load(ctx.h, os.fsencode(load_from), genomic, len(genomic), C.byref(self.h))
            if rc != PGPU_OK:
                raise PgpuError(rc, "index file %s does not fit this sequence" % load_from)

    def save(self, path):
        self.ctx.check(self.ctx.L.pgpu_index_save(self.ctx.h, self.h, self.genomic, os.fsencode(path)))

    def suffix_array(self):
        import numpy as np
        sa = np.empty(self.n, dtype=np.uint32)
        self.ctx.check(self.ctx.L.pgpu_index_suffix_array(
            self.ctx.h, self.h, sa.ctypes.data_as(C.POINTER(C.c_uint32)), self.n))
        return sa

    def find_raw(self, blob: bytes, queries, n_queries: int, out=None):
        """One pgpu_index_find call as it is: `queries` a ctypes array of FindQuery over the pattern bytes `blob`,
        `out` a numpy uint32 array or None (counts alone).  Returns (rc, first[n_queries + 1], total)."""
        import numpy as np
        first = np.zeros(n_queries + 1, dtype=np.uint64)
        total = C.c_size_t(0)
        rc = self.ctx.L.pgpu_index_find(
            self.ctx.h, self.h, blob, len(blob), queries, n_queries,
            out.ctypes.data_as(C.POINTER(C.c_uint32)) if out is not None else None, len(out) if out is not None else 0,
            first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
        return rc, first, total.value

    def find(self, patterns, windows=None):
        """Exact occurrences (byte equality, no N wildcard) of every pattern inside its window (lo, hi) of the
        sequence -- the whole sequence when windows is None: a list of ascending numpy uint32 arrays."""
        import numpy as np
        n = len(patterns)
        if windows is None:
            windows = [(0, self.n)] * n
        if len(windows) != n:
            raise ValueError("one window per pattern")
        lens = np.fromiter((len(p) for p in patterns), dtype=np.uint64, count=n)
        offs = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=offs[1:])
        q = np.zeros(n, dtype=np.dtype([("pat_off", "<u8"), ("pat_len", "<u4"), ("reserved", "<u4"),
                                        ("lo", "<u4"), ("hi", "<u4")]))
        q["pat_off"], q["pat_len"] = offs[:n], lens
        if n:
            w = np.asarray(windows, dtype=np.uint32).reshape(n, 2)
            q["lo"], q["hi"] = w[:, 0], w[:, 1]
        blob = b"".join(patterns)
        qs = q.ctypes.data_as(C.POINTER(FindQuery))
        rc, first, total = self.find_raw(blob, qs, n)             # counts, then the positions
        if rc == PGPU_ENOSPC:
            out = np.empty(total, dtype=np.uint32)
            rc, first, total = self.find_raw(blob, qs, n, out)
        else:
            out = np.empty(0, dtype=np.uint32)
        self.ctx.check(rc)
        return [out[int(first[i]):int(first[i + 1])] for i in range(n)]

    def find_kernel_ms(self):
        """HIP-event times of the last find on this thread: {"count+scan": ms, "fill": ms}"""
        return {"count+scan": self.ctx.L.pgpu_index_find_kernel_ms(0), "fill": self.ctx.L.pgpu_index_find_kernel_ms(1)}

    def classify(self, starts, ends, ctx=None):
        """Class of every intron [starts[i], ends[i]] (both inclusive): numpy uint8, 0 U12, 1 U2, 2 not classified.
        `ctx`: another context that shares this index (default: the one it was made on)."""
        import numpy as np
        ctx = ctx or self.ctx
        iv = np.empty((len(starts), 2), dtype=np.uint32)
        iv[:, 0], iv[:, 1] = starts, ends
        out = np.empty(len(iv), dtype=np.uint8)
        ctx.check(ctx.L.pgpu_index_classify(ctx.h, self.h, iv.ctypes.data_as(C.POINTER(Intron)), len(iv),
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def score5(self, k):
        """The table of 5' splice-site matrix k (0..3): n + 1 float64, what GetScoreOf5Prime*BySS gives per start."""
        import numpy as np
        out = np.empty(self.n + 1, dtype=np.float64)
        self.ctx.check(self.ctx.L.pgpu_index_score5(self.ctx.h, self.h, k, out.ctypes.data_as(C.POINTER(C.c_double)), len(out)))
        return out

    def small_exons_raw(self, ests: bytes, queries, n: int):
        """One pgpu_index_small_exons call as it is: `queries` a numpy array of SEXON_QUERY_DTYPE (or a ctypes array of
        SexonQuery).  Returns (rc, results as a numpy array of SEXON_RESULT_DTYPE)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(SEXON_RESULT_DTYPE))
        qp = queries.ctypes.data_as(C.POINTER(SexonQuery)) if hasattr(queries, "ctypes") else queries
        rc = self.ctx.L.pgpu_index_small_exons(self.ctx.h, self.h, ests, len(ests), qp, n,
                                               res.ctypes.data_as(C.POINTER(SexonResult)))
        return rc, res

    def small_exons(self, ests: bytes, queries):
        """The search loop of search_small_exon for every query: `queries` an iterable of
        (e_off, elen, allgstart, allglen, f1slen, f2plen, min_intron_len) or a numpy array of SEXON_QUERY_DTYPE;
        a numpy array of SEXON_RESULT_DTYPE comes back."""
        import numpy as np
        if not isinstance(queries, np.ndarray):
            rows = list(queries)
            q = np.zeros(len(rows), dtype=np.dtype(SEXON_QUERY_DTYPE))
            for i, r in enumerate(rows):
                q[i] = tuple(r) + (0, 0)
            queries = q
        rc, res = self.small_exons_raw(ests, queries, len(queries))
        self.ctx.check(rc)
        return res

    def small_exons_kernel_ms(self):
        return self.ctx.L.pgpu_index_small_exons_kernel_ms()

    def refine_introns_raw(self, ests: bytes, rows: bytes, queries, n: int):
        """One pgpu_index_refine_introns call as it is: `queries` a numpy array of REFINE_QUERY_DTYPE (or a ctypes array
        of RefineQuery).  Returns (rc, results as a numpy array of REFINE_RESULT_DTYPE)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(REFINE_RESULT_DTYPE))
        qp = queries.ctypes.data_as(C.POINTER(RefineQuery)) if hasattr(queries, "ctypes") else queries
        rc = self.ctx.L.pgpu_index_refine_introns(self.ctx.h, self.h, ests, len(ests), rows, len(rows), qp, n,
                                                  res.ctypes.data_as(C.POINTER(RefineResult)))
        return rc, res

    def refine_introns(self, ests: bytes, rows: bytes, queries):
        """refine_intron's decision for every query from its gap alignment (the rows and v[1..5] of a PGPU_DP_GAP job):
        `queries` a numpy array of REFINE_QUERY_DTYPE; a numpy array of REFINE_RESULT_DTYPE comes back."""
        rc, res = self.refine_introns_raw(ests, rows, queries, len(queries))
        self.ctx.check(rc)
        return res

    def refine_introns_kernel_ms(self):
        return self.ctx.L.pgpu_index_refine_introns_kernel_ms()

    def _chained_raw(self, fn, query_struct, result_struct, result_dtype, ests, exons, queries, n):
        """a chained entry (one query = one list of exons) as it is: (rc, out_exons, one byte per exon, results)"""
        import numpy as np
        out_exons = np.zeros(len(exons), dtype=np.dtype(FACTOR_DTYPE))
        out_bytes = np.zeros(len(exons), dtype=np.uint8)
        res = np.zeros(n, dtype=np.dtype(result_dtype))
        rc = fn(self.ctx.h, self.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(Factor)), len(exons),
                queries.ctypes.data_as(C.POINTER(query_struct)), n, out_exons.ctypes.data_as(C.POINTER(Factor)),
                out_bytes.ctypes.data_as(C.POINTER(C.c_uint8)), res.ctypes.data_as(C.POINTER(result_struct)))
        return rc, out_exons, out_bytes, res

    def refine_chains_raw(self, ests: bytes, exons, queries, n: int):
        """One pgpu_index_refine_chains call as it is: `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        CHAIN_QUERY_DTYPE.  Returns (rc, out_exons, out_steps, results as a numpy array of CHAIN_RESULT_DTYPE)."""
        return self._chained_raw(self.ctx.L.pgpu_index_refine_chains, ChainQuery, ChainResult, CHAIN_RESULT_DTYPE,
                                 ests, exons, queries, n)

    def refine_chains(self, ests: bytes, exons, queries):
        """The reference's refinement loop over every factorization `queries` names (windows, gap alignment and border
        decision per intron, chained on the device): (out_exons, out_steps, results) as numpy arrays."""
        rc, out_exons, out_steps, res = self.refine_chains_raw(ests, exons, queries, len(queries))
        self.ctx.check(rc)
        return out_exons, out_steps, res

    def refine_chains_kernel_ms(self):
        return self.ctx.L.pgpu_index_refine_chains_kernel_ms()

    def clean_chains_raw(self, ests: bytes, exons, queries, n: int):
        """One pgpu_index_clean_chains call as it is: `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        CLEAN_QUERY_DTYPE.  Returns (rc, out_exons, out_marks, results as a numpy array of CLEAN_RESULT_DTYPE)."""
        return self._chained_raw(self.ctx.L.pgpu_index_clean_chains, CleanQuery, CleanResult, CLEAN_RESULT_DTYPE,
                                 ests, exons, queries, n)

    def clean_chains(self, ests: bytes, exons, queries):
        """The reference's cleaning steps over every candidate factorization `queries` names (end-exon alignments and
        trimming, external exons, dust, banded edit distances, coverage, chained on the device): (out_exons, out_marks,
        results) as numpy arrays."""
        rc, out_exons, out_marks, res = self.clean_chains_raw(ests, exons, queries, len(queries))
        self.ctx.check(rc)
        return out_exons, out_marks, res

    def clean_chains_kernel_ms(self):
        return self.ctx.L.pgpu_index_clean_chains_kernel_ms()

    def gap_chains_raw(self, ests: bytes, exons, queries, n: int):
        """One pgpu_index_gap_chains call as it is: `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        GAPS_QUERY_DTYPE.  Returns (rc, out_exons, out_steps, results as a numpy array of GAPS_RESULT_DTYPE)."""
        return self._chained_raw(self.ctx.L.pgpu_index_gap_chains, GapsQuery, GapsResult, GAPS_RESULT_DTYPE,
                                 ests, exons, queries, n)

    def gap_chains(self, ests: bytes, exons, queries):
        """The reference's check_gap_errors over every factorization `queries` names (a border refinement per unaligned
        EST gap, the four ends moved, the distances summed, close exons merged, chained on the device): (out_exons,
        out_steps, results) as numpy arrays."""
        rc, out_exons, out_steps, res = self.gap_chains_raw(ests, exons, queries, len(queries))
        self.ctx.check(rc)
        return out_exons, out_steps, res

    def gap_chains_kernel_ms(self):
        return self.ctx.L.pgpu_index_gap_chains_kernel_ms()

    def tail_chains_raw(self, ests: bytes, exons, queries, n: int, wide: bool = False):
        """One pgpu_index_tail_chains call as it is (wide: pgpu_index_tail_chains_wide): `exons` a numpy array of
        FACTOR_DTYPE, `queries` one of TAIL_QUERY_DTYPE.  Returns (rc, out_exons, out_steps, results as a numpy array of
        TAIL_RESULT_DTYPE)."""
        fn = self.ctx.L.pgpu_index_tail_chains_wide if wide else self.ctx.L.pgpu_index_tail_chains
        return self._chained_raw(fn, TailQuery, TailResult, TAIL_RESULT_DTYPE,
                                 ests, exons, queries, n)

    def tail_chains(self, ests: bytes, exons, queries, wide: bool = False):
        """What est-fact does to every factorization `queries` names directly behind the refinement loop (tail correction,
        polyA, validity, lost prefix and suffix, false small exons, chained on the device): (out_exons, out_steps,
        results) as numpy arrays.  wide: lost windows of up to 1024 EST bytes (pgpu_index_tail_chains_wide)."""
        rc, out_exons, out_steps, res = self.tail_chains_raw(ests, exons, queries, len(queries), wide)
        self.ctx.check(rc)
        return out_exons, out_steps, res

    def tail_chains_kernel_ms(self):
        return self.ctx.L.pgpu_index_tail_chains_kernel_ms()

    def small_chains_raw(self, ests: bytes, exons, queries, n: int, min_intron_length: int, params_reserved: int = 0,
                         no_params: bool = False, wide: bool = False):
        """One pgpu_index_small_chains call as it is (wide: pgpu_index_small_chains_wide): `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        SMALL_QUERY_DTYPE.  Returns (rc, out_exons, out_steps, results as a numpy array of SMALL_RESULT_DTYPE); the two
        output arrays have 2 * len(exons) entries, a query's list at 2 * first_exon."""
        import numpy as np
        out_exons = np.zeros(2 * len(exons), dtype=np.dtype(FACTOR_DTYPE))
        out_steps = np.zeros(2 * len(exons), dtype=np.uint8)
        res = np.zeros(n, dtype=np.dtype(SMALL_RESULT_DTYPE))
        prm = SmallParams(min_intron_length, params_reserved)
        fn = self.ctx.L.pgpu_index_small_chains_wide if wide else self.ctx.L.pgpu_index_small_chains
        rc = fn(self.ctx.h, self.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(Factor)),
                len(exons), queries.ctypes.data_as(C.POINTER(SmallQuery)), n,
                None if no_params else C.byref(prm),
                out_exons.ctypes.data_as(C.POINTER(Factor)),
                out_steps.ctypes.data_as(C.POINTER(C.c_uint8)),
                res.ctypes.data_as(C.POINTER(SmallResult)))
        return rc, out_exons, out_steps, res

    def small_chains(self, ests: bytes, exons, queries, min_intron_length: int, wide: bool = False):
        """The last steps of the reference's refine_EST_factorizations over every factorization `queries` names (a new small
        exon in front of the first exon and between every two, then the last cleaning on the original sequence, chained on
        the device): (out_exons, out_steps, results) as numpy arrays, the first two of 2 * len(exons) entries."""
        rc, out_exons, out_steps, res = self.small_chains_raw(ests, exons, queries, len(queries), min_intron_length, wide=wide)
        self.ctx.check(rc)
        return out_exons, out_steps, res

    def small_chains_kernel_ms(self):
        return self.ctx.L.pgpu_index_small_chains_kernel_ms()

    def candidates_raw(self, records: bytes, rec_first, n: int, min_factor_len, min_intron_length, exons_cap: int):
        """One pgpu_index_candidates call as it is: `records` the concatenated MEG records, `rec_first` a numpy uint64 array
        of n + 1 offsets.  Returns (rc, results as a numpy array of CAND_RESULT_DTYPE, exons (exons_cap entries), n_exons)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(CAND_RESULT_DTYPE))
        exons = np.zeros(exons_cap, dtype=np.dtype(FACTOR_DTYPE))
        prm = CandParams(min_factor_len, min_intron_length)
        total = C.c_size_t(0)
        rc = self.ctx.L.pgpu_index_candidates(self.ctx.h, self.h, records, len(records), rec_first.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              n, C.byref(prm), res.ctypes.data_as(C.POINTER(CandResult)),
                                              exons.ctypes.data_as(C.POINTER(Factor)), exons_cap, C.byref(total))
        return rc, res, exons, total.value

    def candidates(self, records, min_factor_len=15, min_intron_length=40):
        """The candidate factorization of every MEG record of the list `records` (bytes each, as PairingPlan.fetch_meg
        returns them) that is one path: (results as a numpy array of CAND_RESULT_DTYPE, exons as one of FACTOR_DTYPE)."""
        import numpy as np
        first = np.zeros(len(records) + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in records], out=first[1:])
        blob = b"".join(records)
        rc, res, exons, total = self.candidates_raw(blob, first, len(records), min_factor_len, min_intron_length, 0)
        if rc == PGPU_ENOSPC:
            rc, res, exons, total = self.candidates_raw(blob, first, len(records), min_factor_len, min_intron_length, total)
        self.ctx.check(rc)
        return res, exons[:total]

    def candidates_kernel_ms(self):
        return self.ctx.L.pgpu_index_candidates_kernel_ms()

    def candidate_lists_raw(self, records: bytes, rec_first, n: int, min_factor_len, min_intron_length, cands_cap: int, exons_cap: int):
        """One pgpu_index_candidate_lists call as it is (the arguments of candidates_raw).  Returns (rc, results as a numpy array
        of ENUM_RESULT_DTYPE, candidates (cands_cap entries of ENUM_CANDIDATE_DTYPE), exons (exons_cap entries), n_cands,
        n_exons)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(ENUM_RESULT_DTYPE))
        cands = np.zeros(cands_cap, dtype=np.dtype(ENUM_CANDIDATE_DTYPE))
        exons = np.zeros(exons_cap, dtype=np.dtype(FACTOR_DTYPE))
        prm = CandParams(min_factor_len, min_intron_length)
        nc, ne = C.c_size_t(0), C.c_size_t(0)
        rc = self.ctx.L.pgpu_index_candidate_lists(
            self.ctx.h, self.h, records, len(records), rec_first.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(prm),
            res.ctypes.data_as(C.POINTER(EnumResult)), cands.ctypes.data_as(C.POINTER(EnumCandidate)), cands_cap,
            exons.ctypes.data_as(C.POINTER(Factor)), exons_cap, C.byref(nc), C.byref(ne))
        return rc, res, cands, exons, nc.value, ne.value

    def candidate_lists(self, records, min_factor_len=15, min_intron_length=40):
        """Every candidate factorization of every MEG record of the list `records`: (results as a numpy array of
        ENUM_RESULT_DTYPE, candidates as one of ENUM_CANDIDATE_DTYPE, exons as one of FACTOR_DTYPE)."""
        import numpy as np
        first = np.zeros(len(records) + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in records], out=first[1:])
        blob = b"".join(records)
        rc, res, cands, exons, nc, ne = self.candidate_lists_raw(blob, first, len(records), min_factor_len, min_intron_length, 0, 0)
        if rc == PGPU_ENOSPC:
            rc, res, cands, exons, nc, ne = self.candidate_lists_raw(blob, first, len(records), min_factor_len, min_intron_length, nc, ne)
        self.ctx.check(rc)
        return res, cands[:nc], exons[:ne]

    def candidate_lists_kernel_ms(self):
        return self.ctx.L.pgpu_index_candidate_lists_kernel_ms()

    def factorizations_raw(self, ests: bytes, exons, queries, n: int, params, cap: int):
        """One pgpu_index_factorizations call as it is: `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        FACT_QUERY_DTYPE, `params` a FactParams.  Returns (rc, results as a numpy array of FACT_RESULT_DTYPE, exons and step
        bytes (cap entries each), n_out)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(FACT_RESULT_DTYPE))
        out_exons = np.zeros(cap, dtype=np.dtype(FACTOR_DTYPE))
        out_steps = np.zeros(cap, dtype=np.uint8)
        total = C.c_size_t(0)
        rc = self.ctx.L.pgpu_index_factorizations(
            self.ctx.h, self.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(Factor)), len(exons),
            queries.ctypes.data_as(C.POINTER(FactQuery)), n, C.byref(params), res.ctypes.data_as(C.POINTER(FactResult)),
            out_exons.ctypes.data_as(C.POINTER(Factor)), out_steps.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(total))
        return rc, res, out_exons, out_steps, total.value

    def factorizations(self, ests: bytes, exons, queries, complexity_threshold=20.0, suffpref_length_on_est=30,
                       suffpref_length_for_intron=70, suffpref_length_on_gen=30, min_intron_length=40):
        """Every candidate `queries` names through clean, gaps and refine in one call (n_exons == 0: no candidate):
        (results as a numpy array of FACT_RESULT_DTYPE, the final exons, compact, and their step bytes)."""
        prm = FactParams(complexity_threshold, suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen,
                         min_intron_length)
        rc, res, out_exons, out_steps, total = self.factorizations_raw(ests, exons, queries, len(queries), prm, len(exons))
        self.ctx.check(rc)
        return res, out_exons[:total], out_steps[:total]

    def factorizations_kernel_ms(self):
        return self.ctx.L.pgpu_index_factorizations_kernel_ms()

    def factorization_lists_raw(self, ests: bytes, cands, exons, queries, n: int, params, facts_cap: int, exons_cap: int):
        """One pgpu_index_factorization_lists call as it is: `cands` a numpy array of ENUM_CANDIDATE_DTYPE, `exons` one of
        FACTOR_DTYPE, `queries` one of FLIST_QUERY_DTYPE, `params` a FlistParams.  Returns (rc, results as a numpy array of
        FLIST_RESULT_DTYPE, facts (facts_cap entries of FLIST_FACT_DTYPE), exons and step bytes (exons_cap entries each),
        n_facts, n_exons)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(FLIST_RESULT_DTYPE))
        facts = np.zeros(facts_cap, dtype=np.dtype(FLIST_FACT_DTYPE))
        out_exons = np.zeros(exons_cap, dtype=np.dtype(FACTOR_DTYPE))
        out_steps = np.zeros(exons_cap, dtype=np.uint8)
        nf, ne = C.c_size_t(0), C.c_size_t(0)
        rc = self.ctx.L.pgpu_index_factorization_lists(
            self.ctx.h, self.h, ests, len(ests), cands.ctypes.data_as(C.POINTER(EnumCandidate)), len(cands),
            exons.ctypes.data_as(C.POINTER(Factor)), len(exons), queries.ctypes.data_as(C.POINTER(FlistQuery)), n, C.byref(params),
            res.ctypes.data_as(C.POINTER(FlistResult)), facts.ctypes.data_as(C.POINTER(FlistFact)), facts_cap,
            out_exons.ctypes.data_as(C.POINTER(Factor)), out_steps.ctypes.data_as(C.POINTER(C.c_uint8)), exons_cap,
            C.byref(nf), C.byref(ne))
        return rc, res, facts, out_exons, out_steps, nf.value, ne.value

    def factorization_lists(self, ests: bytes, cands, exons, queries, params=None):
        """Every EST `queries` names, from its candidates to its list of factorizations, in one call: (results as a numpy
        array of FLIST_RESULT_DTYPE, facts as one of FLIST_FACT_DTYPE, the final exons, compact, and their step bytes)."""
        prm = params if params is not None else flist_params()
        rc, res, facts, out_exons, out_steps, nf, ne = self.factorization_lists_raw(ests, cands, exons, queries, len(queries), prm,
                                                                                    len(cands), len(exons))
        self.ctx.check(rc)
        return res, facts[:nf], out_exons[:ne], out_steps[:ne]

    def factorization_lists_kernel_ms(self):
        return self.ctx.L.pgpu_index_factorization_lists_kernel_ms()

    def final_factorizations_raw(self, ests: bytes, exons, queries, n: int, params, small_params, cap: int, wide: bool = False):
        """One pgpu_index_final_factorizations call as it is (wide: pgpu_index_final_factorizations_wide): `exons` a numpy array of FACTOR_DTYPE, `queries` one of
        FINAL_QUERY_DTYPE, `params` a FactParams, `small_params` a SmallParams or None.  Returns (rc, results as a numpy array
        of FINAL_RESULT_DTYPE, exons and step bytes (cap entries each), n_out)."""
        import numpy as np
        res = np.zeros(n, dtype=np.dtype(FINAL_RESULT_DTYPE))
        out_exons = np.zeros(cap, dtype=np.dtype(FACTOR_DTYPE))
        out_steps = np.zeros(cap, dtype=np.uint8)
        total = C.c_size_t(0)
        fn = self.ctx.L.pgpu_index_final_factorizations_wide if wide else self.ctx.L.pgpu_index_final_factorizations
        rc = fn(
            self.ctx.h, self.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(Factor)), len(exons),
            queries.ctypes.data_as(C.POINTER(FinalQuery)), n, C.byref(params),
            None if small_params is None else C.byref(small_params), res.ctypes.data_as(C.POINTER(FinalResult)),
            out_exons.ctypes.data_as(C.POINTER(Factor)), out_steps.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(total))
        return rc, res, out_exons, out_steps, total.value

    def final_factorizations(self, ests: bytes, exons, queries, complexity_threshold=20.0, suffpref_length_on_est=30,
                             suffpref_length_for_intron=70, suffpref_length_on_gen=30, min_intron_length=40, wide=False):
        """Every candidate `queries` names through clean, gaps, refine, tail and small in one call (n_exons == 0: no
        candidate): (results as a numpy array of FINAL_RESULT_DTYPE, the final exons, compact, and their step bytes)."""
        prm = FactParams(complexity_threshold, suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen,
                         min_intron_length)
        rc, res, out_exons, out_steps, total = self.final_factorizations_raw(ests, exons, queries, len(queries), prm,
                                                                             SmallParams(min_intron_length, 0), 2 * len(exons),
                                                                             wide)
        self.ctx.check(rc)
        return res, out_exons[:total], out_steps[:total]

    def final_factorizations_kernel_ms(self):
        return self.ctx.L.pgpu_index_final_factorizations_kernel_ms()

    def close(self):
        if self.h:
            self.ctx.L.pgpu_index_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


def flist_params(complexity_threshold=20.0, suffpref_length_on_est=30, suffpref_length_for_intron=70, suffpref_length_on_gen=30,
                 min_intron_length=40, max_coverage_diff=0.05, max_site_difference=50, max_gaplength_diff=20,
                 max_number_of_factorizations=0, reserved=0):
    """pgpu_flist_params; the defaults are the reference's configuration (src/options.ggo)"""
    return FlistParams(complexity_threshold, suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen,
                       min_intron_length, max_coverage_diff, max_site_difference, max_gaplength_diff, max_number_of_factorizations,
                       reserved)


def flist_handoffs_probe(ctx, idx, ests, cands, exons, queries, params, gaps_results, gaps_exons, gaps_steps):
    """pgpu_flist_handoffs_probe (pintron_amd/csrc/pgpu_flists.hip; no part of the C-ABI's header):
    pgpu_index_factorization_lists with gaps_kernel's three outputs given -- `gaps_results` a numpy array of GAPS_RESULT_DTYPE
    with one entry per candidate, `gaps_exons` (FACTOR_DTYPE) and `gaps_steps` (uint8) with len(exons) + len(cands) entries
    each -- instead of computed.  Returns (rc, results, facts, exons, steps)."""
    import numpy as np
    assert len(gaps_results) == len(cands) and len(gaps_exons) == len(gaps_steps) == len(exons) + len(cands)
    sz = C.c_size_t
    f = ctx.L.pgpu_flist_handoffs_probe
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, sz, C.POINTER(EnumCandidate), sz, C.POINTER(Factor), sz, C.POINTER(FlistQuery), sz,
                  C.POINTER(FlistParams), C.POINTER(FlistResult), C.POINTER(FlistFact), sz, C.POINTER(Factor), C.POINTER(C.c_uint8), sz,
                  C.POINTER(sz), C.POINTER(sz), C.POINTER(GapsResult), C.POINTER(Factor), C.POINTER(C.c_uint8)]
    n = len(queries)
    res = np.zeros(n, dtype=np.dtype(FLIST_RESULT_DTYPE))
    facts = np.zeros(len(cands), dtype=np.dtype(FLIST_FACT_DTYPE))
    out_exons = np.zeros(len(exons), dtype=np.dtype(FACTOR_DTYPE))
    out_steps = np.zeros(len(exons), dtype=np.uint8)
    nf, ne = sz(0), sz(0)
    rc = f(ctx.h, idx.h, ests, len(ests), cands.ctypes.data_as(C.POINTER(EnumCandidate)), len(cands),
           exons.ctypes.data_as(C.POINTER(Factor)), len(exons), queries.ctypes.data_as(C.POINTER(FlistQuery)), n, C.byref(params),
           res.ctypes.data_as(C.POINTER(FlistResult)), facts.ctypes.data_as(C.POINTER(FlistFact)), len(facts),
           out_exons.ctypes.data_as(C.POINTER(Factor)), out_steps.ctypes.data_as(C.POINTER(C.c_uint8)), len(out_exons),
           C.byref(nf), C.byref(ne), gaps_results.ctypes.data_as(C.POINTER(GapsResult)), gaps_exons.ctypes.data_as(C.POINTER(Factor)),
           gaps_steps.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, res, facts[:nf.value], out_exons[:ne.value], out_steps[:ne.value]


def final_handoffs_probe(ctx, tlen, ests_len, q, fres, fex, tres, tex, tst, sres, sex, sst):
    """pgpu_final_handoffs_probe (pintron_amd/csrc/pgpu_final.hip; no part of the C-ABI's header): the three hand-off kernels
    of the final stage over stage results the caller made, numpy arrays in the layouts of the driver's block.  Returns (rc,
    tail queries, small queries, small's input exons, results, exons, steps)."""
    import numpy as np
    n, E = len(q), len(fex)
    tq = np.zeros(n, dtype=np.dtype(TAIL_QUERY_DTYPE))
    sq = np.zeros(n, dtype=np.dtype(SMALL_QUERY_DTYPE))
    ex_sin = np.zeros(E + n, dtype=np.dtype(FACTOR_DTYPE))
    res = np.zeros(n, dtype=np.dtype(FINAL_RESULT_DTYPE))
    out_exons = np.zeros(2 * E, dtype=np.dtype(FACTOR_DTYPE))
    out_steps = np.zeros(2 * E, dtype=np.uint8)
    total = C.c_size_t(0)
    f = ctx.L.pgpu_final_handoffs_probe
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 12 + \
        [C.POINTER(C.c_size_t)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = f(ctx.h, tlen, ests_len, p(q), n, p(fres), p(fex), E, p(tres), p(tex), p(tst), p(sres), p(sex), p(sst), p(tq), p(sq), p(ex_sin),
           p(res), p(out_exons), p(out_steps), C.byref(total))
    return rc, tq, sq, ex_sin, res, out_exons[:total.value], out_steps[:total.value]


def unit_params(pref_N_length=0, retain_externals=1, reserved=(0, 0, 0)):
    return UnitParams(pref_N_length, retain_externals, (C.c_uint8 * 3)(*reserved))


def unit_records_raw(ctx, res, exons, empty_graph, queries, n, params, blob_cap, n_pat=None):
    """One pgpu_unit_records call as it is: `res` a numpy array of FINAL_RESULT_DTYPE (one per pattern), `exons` one of
    FACTOR_DTYPE, `empty_graph` a numpy uint8 array with a byte per pattern or None, `queries` one of UNIT_QUERY_DTYPE,
    `params` a UnitParams.  Returns (rc, results as a numpy array of UNIT_RESULT_DTYPE, the blob (blob_cap bytes), blob_len)."""
    import numpy as np
    out = np.zeros(min(n, len(queries)), dtype=np.dtype(UNIT_RESULT_DTYPE))      # (n beyond the queries: a call to be refused)
    blob = np.zeros(blob_cap, dtype=np.uint8)
    total = C.c_size_t(0)
    rc = ctx.L.pgpu_unit_records(
        ctx.h, res.ctypes.data_as(C.POINTER(FinalResult)), len(res) if n_pat is None else n_pat,
        exons.ctypes.data_as(C.POINTER(Factor)), len(exons),
        None if empty_graph is None else empty_graph.ctypes.data_as(C.POINTER(C.c_uint8)),
        queries.ctypes.data_as(C.POINTER(UnitQuery)), n, C.byref(params), out.ctypes.data_as(C.POINTER(UnitResult)),
        blob.ctypes.data_as(C.c_void_p), blob_cap, C.byref(total))
    return rc, out, blob, total.value


def unit_records(ctx, res, exons, empty_graph, queries, pref_N_length=0, retain_externals=True):
    """The verdict of every unit `queries` names over the finals (res, exons) and the groups of the ALIGNED ones:
    (results as a numpy array of UNIT_RESULT_DTYPE, the blob as bytes)."""
    cap = 12 * len(queries) + 16 * int(res["n_exons"][res["outcome"] == FACT_DONE].sum())
    rc, out, blob, total = unit_records_raw(ctx, res, exons, empty_graph, queries, len(queries),
                                            unit_params(pref_N_length, int(bool(retain_externals))), cap)
    ctx.check(rc)
    return out, blob[:total].tobytes()


def _offsets(parts):
    """the bytes of `parts` joined, and their len(parts) + 1 offsets as a numpy uint64 array"""
    import numpy as np
    first = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        np.cumsum([len(x) for x in parts], out=first[1:])
    return b"".join(parts), first


def unit_texts_raw(ctx, units, n, blob, headers, hdr_first, seqs, seq_first, n_pat, genomic, raw_cap, pests_cap,
                   blob_len=None, headers_len=None, seqs_len=None):
    """One pgpu_unit_texts call as it is: `units` a numpy array of UNIT_RESULT_DTYPE, `blob`, `headers`, `seqs`, `genomic`
    bytes, `hdr_first` and `seq_first` numpy uint64 arrays.  Returns (rc, results as a numpy array of TEXT_RESULT_DTYPE, raw
    and pests as numpy uint8 arrays of their caps, raw_len, pests_len)."""
    import numpy as np
    out = np.zeros(min(n, len(units)), dtype=np.dtype(TEXT_RESULT_DTYPE))
    raw, pests = np.zeros(raw_cap, dtype=np.uint8), np.zeros(pests_cap, dtype=np.uint8)
    raw_len, pests_len = C.c_size_t(0), C.c_size_t(0)
    b = lambda x: C.cast(C.c_char_p(x), C.c_void_p)
    rc = ctx.L.pgpu_unit_texts(
        ctx.h, units.ctypes.data_as(C.POINTER(UnitResult)), n, b(blob), len(blob) if blob_len is None else blob_len,
        b(headers), len(headers) if headers_len is None else headers_len, hdr_first.ctypes.data_as(C.POINTER(C.c_uint64)),
        b(seqs), len(seqs) if seqs_len is None else seqs_len, seq_first.ctypes.data_as(C.POINTER(C.c_uint64)), n_pat,
        b(genomic), len(genomic), out.ctypes.data_as(C.POINTER(TextResult)),
        raw.ctypes.data_as(C.c_void_p), raw_cap, C.byref(raw_len), pests.ctypes.data_as(C.c_void_p), pests_cap, C.byref(pests_len))
    return rc, out, raw, pests, raw_len.value, pests_len.value


def unit_texts(ctx, units, blob, headers, seqs, genomic):
    """The two texts of every ALIGNED unit: `units` a numpy array of UNIT_RESULT_DTYPE over `blob`, `headers` one bytes per
    unit, `seqs` one bytes per pattern, `genomic` the original genomic sequence -> (results as a numpy array of
    TEXT_RESULT_DTYPE, raw as bytes, pests as bytes).  Two calls: the first one asks for the sizes."""
    hb, hf = _offsets(headers)
    sb, sf = _offsets(seqs)
    args = (ctx, units, len(units), blob, hb, hf, sb, sf, len(seqs), genomic)
    rc, out, raw, pests, raw_len, pests_len = unit_texts_raw(*args, 0, 0)
    if rc == PGPU_ENOSPC:
        rc, out, raw, pests, raw_len, pests_len = unit_texts_raw(*args, raw_len, pests_len)
    ctx.check(rc)
    return out, raw[:raw_len].tobytes(), pests[:pests_len].tobytes()


def unit_sides_raw(ctx, q, units, n, recs, rec_first, n_pat, headers, hdr_first, seqs, seq_first, caps,
                   recs_len=None, headers_len=None, seqs_len=None):
    """One pgpu_unit_sides call as it is: `q` a numpy array of UNIT_QUERY_DTYPE, `units` one of UNIT_RESULT_DTYPE, `recs`,
    `headers`, `seqs` bytes, `rec_first`, `hdr_first` and `seq_first` numpy uint64 arrays, `caps` the three caps.  Returns
    (rc, results as a numpy array of SIDE_RESULT_DTYPE, the three blobs as numpy uint8 arrays of their caps, the three
    lengths)."""
    import numpy as np
    out = np.zeros(min(n, len(units)), dtype=np.dtype(SIDE_RESULT_DTYPE))
    blobs = [np.zeros(c, dtype=np.uint8) for c in caps]
    lens = (C.c_size_t * 3)(0, 0, 0)
    b = lambda x: C.cast(C.c_char_p(x), C.c_void_p)
    rc = ctx.L.pgpu_unit_sides(
        ctx.h, q.ctypes.data_as(C.POINTER(UnitQuery)), units.ctypes.data_as(C.POINTER(UnitResult)), n,
        b(recs), len(recs) if recs_len is None else recs_len, rec_first.ctypes.data_as(C.POINTER(C.c_uint64)), n_pat,
        b(headers), len(headers) if headers_len is None else headers_len, hdr_first.ctypes.data_as(C.POINTER(C.c_uint64)),
        b(seqs), len(seqs) if seqs_len is None else seqs_len, seq_first.ctypes.data_as(C.POINTER(C.c_uint64)),
        out.ctypes.data_as(C.POINTER(SideResult)), blobs[0].ctypes.data_as(C.c_void_p), caps[0],
        blobs[1].ctypes.data_as(C.c_void_p), caps[1], blobs[2].ctypes.data_as(C.c_void_p), caps[2], lens)
    return rc, out, blobs, tuple(lens)


def unit_sides(ctx, q, units, records, headers, seqs):
    """The three side texts of every settled unit: `q` and `units` numpy arrays of UNIT_QUERY_DTYPE and UNIT_RESULT_DTYPE,
    `records` one bytes per pattern (as PairingPlan.fetch_meg gives them), `headers` one bytes per unit, `seqs` one
    (original) sequence per pattern -> (results as a numpy array of SIDE_RESULT_DTYPE, megs, pmegs, edges as bytes).  Two
    calls: the first one asks for the sizes."""
    rb, rf = _offsets(records)
    hb, hf = _offsets(headers)
    sb, sf = _offsets(seqs)
    args = (ctx, q, units, len(units), rb, rf, len(records), hb, hf, sb, sf)
    rc, out, blobs, lens = unit_sides_raw(*args, (0, 0, 0))
    if rc == PGPU_ENOSPC:
        rc, out, blobs, lens = unit_sides_raw(*args, lens)
    ctx.check(rc)
    return (out,) + tuple(b[:n].tobytes() for b, n in zip(blobs, lens))


class TextSource:
    """The original genomic sequence in HBM, for PairingPlan.run_texts"""

    def __init__(self, ctx, genomic: bytes):
        self.ctx, self.h = ctx, C.c_void_p()
        ctx.check(ctx.L.pgpu_text_source_create(ctx.h, genomic, len(genomic), C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.L.pgpu_text_source_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class MegParams(C.Structure):       # pgpu_meg_params; defaults = src/options.ggo:94-370
    _fields_ = [("min_factor_len", C.c_uint32), ("min_intron_length", C.c_int32), ("max_intron_length", C.c_int32),
                ("max_pairings_in_MEG", C.c_uint32), ("max_prefix_discarded_rate", C.c_double),
                ("max_suffix_discarded_rate", C.c_double), ("max_freq_shortest_pairing", C.c_double),
                ("trans_red", C.c_uint32), ("short_edge_comp", C.c_uint32)]


def parse_meg_record(rec: bytes):
    """One record of pgpu_pairing_plan_fetch_meg -> dict(flags, vertices [(p,t,l)], adj [[targets]],
    meg_text, edges_text); vertices/adj are empty for an unavailable record."""
    import struct
    nv, ne, flags, _ = struct.unpack_from("<4I", rec, 0)
    if flags & 2:
        return dict(flags=flags, vertices=[], adj=[], meg_text=b"", edges_text=b"")
    verts = [struct.unpack_from("<3i", rec, 16 + 12 * k) for k in range(nv)]
    first = struct.unpack_from("<%dH" % (nv + 1), rec, 16 + 12 * nv)
    base = 16 + 12 * nv + 2 * (nv + 1)
    adj = [list(rec[base + first[k]:base + first[k + 1]]) for k in range(nv)]
    graph = (base + ne + 3) & ~3
    ml, el = struct.unpack_from("<2I", rec, graph)
    return dict(flags=flags, vertices=verts, adj=adj, meg_text=rec[graph + 8:graph + 8 + ml],
                edges_text=rec[graph + 8 + ml:graph + 8 + ml + el])


class PairingPlan:
    """Patterns resident in HBM; run() = all pairing kernels; fetch() -> (triples[n,3], first[n_pat+1]);
    run_meg()/fetch_meg() = the MEG stage behind the pairings."""
    STAGES = ["locate", "chain", "count+scan", "fill", "cross+scan", "emit"]
    _n_units = 0                    # units of the last run_units

    def __init__(self, ctx: Context, index: Index, patterns, resident=False, originals=None):
        """originals: {pattern index: the ORIGINAL sequence of that pattern (the pattern is the working one)}, for the
        patterns where the two differ; only the final stage reads them"""
        import numpy as np
        self.ctx, self.n_pat = ctx, len(patterns)
        self._blob = b"".join(patterns)
        self._off = np.zeros(len(patterns) + 1, dtype=np.uint64)
        np.cumsum([len(p) for p in patterns], out=self._off[1:])
        self.h = C.c_void_p()
        if originals is not None:
            which = sorted(originals)
            rc = self.create_with_originals_raw(ctx, index, self._blob, self._off, self.n_pat, resident,
                                                np.array(which, dtype=np.uint32), [originals[k] for k in which], self.h)
            ctx.check(rc)
            return
        # resident: the buffers a run writes are shared with the context's other resident plans (results valid
        # until another of them runs)
        create = ctx.L.pgpu_pairing_plan_create_resident if resident else ctx.L.pgpu_pairing_plan_create
        ctx.check(create(ctx.h, index.h, self._blob, self._off.ctypes.data_as(C.POINTER(C.c_uint64)),
                         self.n_pat, C.byref(self.h)))

    @staticmethod
    def create_with_originals_raw(ctx, index, blob, off, n_pat, resident, orig_pat, orig_seqs, handle, null_lists=False):
        """One pgpu_pairing_plan_create_with_originals call as it is: orig_pat a numpy uint32 array, orig_seqs the
        sequences it names.  Returns rc; `handle` (a c_void_p) receives the plan."""
        import numpy as np
        first = np.zeros(len(orig_seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in orig_seqs], out=first[1:])
        return ctx.L.pgpu_pairing_plan_create_with_originals(
            ctx.h, index.h, blob, off.ctypes.data_as(C.POINTER(C.c_uint64)), n_pat, int(resident),
            None if null_lists else orig_pat.ctypes.data_as(C.POINTER(C.c_uint32)),
            None if null_lists else first.ctypes.data_as(C.POINTER(C.c_uint64)), b"".join(orig_seqs), len(orig_seqs),
            C.byref(handle))

    def run(self, min_factor_len=15, rate=0.2):
        prm = PairingParams(min_factor_len, 0, rate)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run(self.ctx.h, self.h, C.byref(prm)))
        return self.ctx.L.pgpu_pairing_plan_count(self.h)

    def stage_ms(self):
        return {s: self.ctx.L.pgpu_pairing_plan_kernel_ms(self.h, k) for k, s in enumerate(self.STAGES)}

    def fetch(self):
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_count(self.h)
        out = np.zeros((max(n, 1), 3), dtype=np.int32)
        first = np.zeros(self.n_pat + 1, dtype=np.uint64)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_fetch(
            self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(Pairing)), n,
            first.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:n], first

    def run_meg(self, min_factor_len=15, min_intron_length=40, max_intron_length=0, max_pairings_in_MEG=80,
                max_prefix_discarded_rate=0.6, max_suffix_discarded_rate=0.6, max_freq_shortest_pairing=0.4,
                trans_red=True, short_edge_comp=True):
        prm = MegParams(min_factor_len, min_intron_length, max_intron_length, max_pairings_in_MEG,
                        max_prefix_discarded_rate, max_suffix_discarded_rate, max_freq_shortest_pairing,
                        int(trans_red), int(short_edge_comp))
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run_meg(self.ctx.h, self.h, C.byref(prm)))
        return self.ctx.L.pgpu_pairing_plan_meg_bytes(self.h)

    def fetch_meg(self):
        """list of raw records (bytes), one per pattern"""
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_meg_bytes(self.h)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        first = np.zeros(self.n_pat + 1, dtype=np.uint64)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_fetch_meg(
            self.ctx.h, self.h, out.ctypes.data_as(C.c_void_p), n, first.ctypes.data_as(C.POINTER(C.c_uint64))))
        raw = out.tobytes()
        return [raw[int(first[i]):int(first[i + 1])] for i in range(self.n_pat)]

    def run_candidates(self, min_factor_len=15, min_intron_length=40):
        """the candidate stage over the records of the last run_meg, which stay in HBM; returns the number of exons"""
        prm = CandParams(min_factor_len, min_intron_length)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run_candidates(self.ctx.h, self.h, C.byref(prm)))
        return self.ctx.L.pgpu_pairing_plan_candidate_exons(self.h)

    def fetch_candidates(self):
        """(results as a numpy array of CAND_RESULT_DTYPE, one per pattern; exons as one of FACTOR_DTYPE)"""
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_candidate_exons(self.h)
        res = np.zeros(self.n_pat, dtype=np.dtype(CAND_RESULT_DTYPE))
        exons = np.zeros(n, dtype=np.dtype(FACTOR_DTYPE))
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_fetch_candidates(
            self.ctx.h, self.h, res.ctypes.data_as(C.POINTER(CandResult)), exons.ctypes.data_as(C.POINTER(Factor)), n))
        return res, exons

    def candidates_ms(self):
        return self.ctx.L.pgpu_pairing_plan_candidates_ms(self.h)

    def run_candidate_lists(self, min_factor_len=15, min_intron_length=40):
        """every candidate of the records of the last run_meg, which stay in HBM; a branch beside the stages: it changes
        nothing of what they hold.  Returns (candidates, exons)."""
        prm = CandParams(min_factor_len, min_intron_length)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run_candidate_lists(self.ctx.h, self.h, C.byref(prm)))
        return self.candidate_list_counts()

    def candidate_list_counts(self):
        nc, ne = C.c_uint64(0), C.c_uint64(0)
        self.ctx.L.pgpu_pairing_plan_candidate_list_counts(self.h, C.byref(nc), C.byref(ne))
        return nc.value, ne.value

    def fetch_candidate_lists(self):
        """(results as a numpy array of ENUM_RESULT_DTYPE, one per pattern; candidates as one of ENUM_CANDIDATE_DTYPE; exons
        as one of FACTOR_DTYPE)"""
        import numpy as np
        nc, ne = self.candidate_list_counts()
        res = np.zeros(self.n_pat, dtype=np.dtype(ENUM_RESULT_DTYPE))
        cands = np.zeros(nc, dtype=np.dtype(ENUM_CANDIDATE_DTYPE))
        exons = np.zeros(ne, dtype=np.dtype(FACTOR_DTYPE))
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_fetch_candidate_lists(
            self.ctx.h, self.h, res.ctypes.data_as(C.POINTER(EnumResult)), cands.ctypes.data_as(C.POINTER(EnumCandidate)), nc,
            exons.ctypes.data_as(C.POINTER(Factor)), ne))
        return res, cands, exons

    def candidate_lists_ms(self):
        return self.ctx.L.pgpu_pairing_plan_candidate_lists_ms(self.h)

    def run_factorizations(self, complexity_threshold=20.0, suffpref_length_on_est=30, suffpref_length_for_intron=70,
                           suffpref_length_on_gen=30, min_intron_length=40):
        """every candidate of the last run_candidates through clean, gaps and refine, where it lies; returns the number of
        exons of the answer"""
        prm = FactParams(complexity_threshold, suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen,
                         min_intron_length)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run_factorizations(self.ctx.h, self.h, C.byref(prm)))
        return self.ctx.L.pgpu_pairing_plan_factorization_exons(self.h)

    def fetch_factorizations(self):
        """(results as a numpy array of FACT_RESULT_DTYPE, one per pattern; the final exons, compact; their step bytes)"""
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_factorization_exons(self.h)
        res = np.zeros(self.n_pat, dtype=np.dtype(FACT_RESULT_DTYPE))
        exons = np.zeros(n, dtype=np.dtype(FACTOR_DTYPE))
        steps = np.zeros(n, dtype=np.uint8)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_fetch_factorizations(
            self.ctx.h, self.h, res.ctypes.data_as(C.POINTER(FactResult)), exons.ctypes.data_as(C.POINTER(Factor)),
            steps.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return res, exons, steps

    def factorizations_ms(self, k=0):
        """HIP-event time of the last run_factorizations: k = 0 the whole call, 1 clean, 2 gaps, 3 refine"""
        return self.ctx.L.pgpu_pairing_plan_factorizations_ms(self.h, k)

    def run_factorization_lists(self, params=None):
        """the candidate lists of the last run_candidate_lists to lists of factorizations, where they lie"""
        prm = params if params is not None else flist_params()
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_run_factorization_lists(self.ctx.h, self.h, C.byref(prm)))
        return self

    def factorization_list_counts(self):
        nf, ne = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self.ctx.L.pgpu_pairing_plan_factorization_list_counts(self.h, C.byref(nf), C.byref(ne)))
        return nf.value, ne.value

    def fetch_factorization_lists_raw(self, facts_cap=None, exons_cap=None):
        import numpy as np
        nf, ne = self.factorization_list_counts()
        facts_cap = nf if facts_cap is None else facts_cap
        exons_cap = ne if exons_cap is None else exons_cap
        res = np.zeros(self.n_pat, dtype=np.dtype(FLIST_RESULT_DTYPE))
        facts = np.zeros(facts_cap, dtype=np.dtype(FLIST_FACT_DTYPE))
        exons = np.zeros(exons_cap, dtype=np.dtype(FACTOR_DTYPE))
        steps = np.zeros(exons_cap, dtype=np.uint8)
        rc = self.ctx.L.pgpu_pairing_plan_fetch_factorization_lists(
            self.ctx.h, self.h, res.ctypes.data_as(C.POINTER(FlistResult)), facts.ctypes.data_as(C.POINTER(FlistFact)), facts_cap,
            exons.ctypes.data_as(C.POINTER(Factor)), steps.ctypes.data_as(C.POINTER(C.c_uint8)), exons_cap)
        return rc, res, facts, exons, steps

    def fetch_factorization_lists(self):
        """(results as a numpy array of FLIST_RESULT_DTYPE, one per pattern; facts as one of FLIST_FACT_DTYPE; the final exons,
        compact; their step bytes)"""
        rc, res, facts, exons, steps = self.fetch_factorization_lists_raw()
        self.ctx.check(rc)
        return res, facts, exons, steps

    def factorization_lists_ms(self, k=0):
        """HIP-event time of the last run_factorization_lists: k = 0 the whole call, 1 clean, 2 select, 3 gaps, 4 refine"""
        return self.ctx.L.pgpu_pairing_plan_factorization_lists_ms(self.h, k)

    def run_final_factorizations_raw(self, min_intron_length=40, reserved=0, no_params=False, wide=False):
        prm = SmallParams(min_intron_length, reserved)
        L = self.ctx.L
        fn = L.pgpu_pairing_plan_run_final_factorizations_wide if wide else L.pgpu_pairing_plan_run_final_factorizations
        return fn(self.ctx.h, self.h, None if no_params else C.byref(prm))

    def run_final_factorizations(self, min_intron_length=40, wide=False):
        """every factorization of the last run_factorizations through tail and small, where it lies (wide: with the wide
        kernels behind the two stage kernels); returns the number of exons of the answer"""
        self.ctx.check(self.run_final_factorizations_raw(min_intron_length, wide=wide))
        return self.ctx.L.pgpu_pairing_plan_final_exons(self.h)

    def fetch_final_factorizations_raw(self, cap=None):
        """(rc, results as a numpy array of FINAL_RESULT_DTYPE, one per pattern; the final exons, compact; their step bytes)"""
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_final_exons(self.h) if cap is None else cap
        res = np.zeros(self.n_pat, dtype=np.dtype(FINAL_RESULT_DTYPE))
        exons = np.zeros(n, dtype=np.dtype(FACTOR_DTYPE))
        steps = np.zeros(n, dtype=np.uint8)
        rc = self.ctx.L.pgpu_pairing_plan_fetch_final_factorizations(
            self.ctx.h, self.h, res.ctypes.data_as(C.POINTER(FinalResult)), exons.ctypes.data_as(C.POINTER(Factor)),
            steps.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        return rc, res, exons, steps

    def fetch_final_factorizations(self):
        rc, res, exons, steps = self.fetch_final_factorizations_raw()
        self.ctx.check(rc)
        return res, exons, steps

    def final_ms(self, k=0):
        """HIP-event time of the last run_final_factorizations: k = 0 the whole call, 1 tail, 2 small"""
        return self.ctx.L.pgpu_pairing_plan_final_ms(self.h, k)

    def run_units_raw(self, queries, n, params):
        """queries: a numpy array of UNIT_QUERY_DTYPE (or None), params: a UnitParams (or None)"""
        return self.ctx.L.pgpu_pairing_plan_run_units(
            self.ctx.h, self.h, None if queries is None else queries.ctypes.data_as(C.POINTER(UnitQuery)), n,
            None if params is None else C.byref(params))

    def run_units(self, queries, pref_N_length=0, retain_externals=True):
        """the finals of the last run_final_factorizations to one verdict per unit and the groups of the ALIGNED ones, where
        they lie; returns the bytes of the blob"""
        self._n_units = len(queries)
        self.ctx.check(self.run_units_raw(queries, len(queries), unit_params(pref_N_length, int(bool(retain_externals)))))
        return self.ctx.L.pgpu_pairing_plan_unit_bytes(self.h)

    def fetch_units_raw(self, n_units, cap=None):
        """(rc, results as a numpy array of UNIT_RESULT_DTYPE, one per unit; the blob as a numpy uint8 array)"""
        import numpy as np
        n = self.ctx.L.pgpu_pairing_plan_unit_bytes(self.h) if cap is None else cap
        out = np.zeros(max(n_units, 1), dtype=np.dtype(UNIT_RESULT_DTYPE))
        blob = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self.ctx.L.pgpu_pairing_plan_fetch_units(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(UnitResult)),
                                                      blob.ctypes.data_as(C.c_void_p), n)
        return rc, out[:n_units], blob[:n]

    def fetch_units(self):
        rc, out, blob = self.fetch_units_raw(self._n_units)
        self.ctx.check(rc)
        return out, blob.tobytes()

    def units_ms(self):
        """HIP-event time of the last run_units (count + scan + write)"""
        return self.ctx.L.pgpu_pairing_plan_units_ms(self.h)

    def run_texts_raw(self, source, headers, headers_len, hdr_first):
        """source: a TextSource (or None), headers: bytes (or None), hdr_first: a numpy uint64 array (or None)"""
        return self.ctx.L.pgpu_pairing_plan_run_texts(
            self.ctx.h, self.h, None if source is None else source.h,
            None if headers is None else C.cast(C.c_char_p(headers), C.c_void_p), headers_len,
            None if hdr_first is None else hdr_first.ctypes.data_as(C.POINTER(C.c_uint64)))

    def run_texts(self, source, headers):
        """the units of the last run_units to est-fact's two texts, where they lie; headers: one bytes per unit
        -> (bytes of raw, bytes of pests)"""
        hb, hf = _offsets(headers)
        self.ctx.check(self.run_texts_raw(source, hb, len(hb), hf))
        return self.text_bytes(0), self.text_bytes(1)

    def text_bytes(self, which):
        return self.ctx.L.pgpu_pairing_plan_text_bytes(self.h, which)

    def fetch_texts_raw(self, n_units, raw_cap=None, pests_cap=None):
        """(rc, results as a numpy array of TEXT_RESULT_DTYPE, one per unit; raw and pests as numpy uint8 arrays)"""
        import numpy as np
        rn = self.text_bytes(0) if raw_cap is None else raw_cap
        pn = self.text_bytes(1) if pests_cap is None else pests_cap
        out = np.zeros(max(n_units, 1), dtype=np.dtype(TEXT_RESULT_DTYPE))
        raw, pests = np.zeros(max(rn, 1), dtype=np.uint8), np.zeros(max(pn, 1), dtype=np.uint8)
        rc = self.ctx.L.pgpu_pairing_plan_fetch_texts(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(TextResult)),
                                                      raw.ctypes.data_as(C.c_void_p), rn, pests.ctypes.data_as(C.c_void_p), pn)
        return rc, out[:n_units], raw[:rn], pests[:pn]

    def fetch_texts(self):
        rc, out, raw, pests = self.fetch_texts_raw(self._n_units)
        self.ctx.check(rc)
        return out, raw.tobytes(), pests.tobytes()

    def texts_ms(self):
        """HIP-event time of the last run_texts (count + scans + write)"""
        return self.ctx.L.pgpu_pairing_plan_texts_ms(self.h)

    def texts_write_ms(self):
        """HIP-event time of the write pass of the last run_texts"""
        return self.ctx.L.pgpu_pairing_plan_texts_write_ms(self.h)

    def run_sides_raw(self):
        return self.ctx.L.pgpu_pairing_plan_run_sides(self.ctx.h, self.h)

    def run_sides(self):
        """the records of the units of the last run_units, with the headers of the last run_texts, to est-fact's three side
        texts, where they lie -> (bytes of megs, of pmegs, of edges)"""
        self.ctx.check(self.run_sides_raw())
        return tuple(self.side_bytes(k) for k in range(3))

    def side_bytes(self, which):
        return self.ctx.L.pgpu_pairing_plan_side_bytes(self.h, which)

    def fetch_sides_raw(self, n_units, caps=None):
        """(rc, results as a numpy array of SIDE_RESULT_DTYPE, one per unit; megs, pmegs and edges as numpy uint8 arrays)"""
        import numpy as np
        caps = [self.side_bytes(k) for k in range(3)] if caps is None else list(caps)
        out = np.zeros(max(n_units, 1), dtype=np.dtype(SIDE_RESULT_DTYPE))
        blobs = [np.zeros(max(c, 1), dtype=np.uint8) for c in caps]
        rc = self.ctx.L.pgpu_pairing_plan_fetch_sides(
            self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(SideResult)), blobs[0].ctypes.data_as(C.c_void_p), caps[0],
            blobs[1].ctypes.data_as(C.c_void_p), caps[1], blobs[2].ctypes.data_as(C.c_void_p), caps[2])
        return rc, out[:n_units], [b[:c] for b, c in zip(blobs, caps)]

    def fetch_sides(self):
        rc, out, blobs = self.fetch_sides_raw(self._n_units)
        self.ctx.check(rc)
        return (out,) + tuple(b.tobytes() for b in blobs)

    def sides_ms(self):
        """HIP-event time of the last run_sides (count + scans + write)"""
        return self.ctx.L.pgpu_pairing_plan_sides_ms(self.h)

    def sides_write_ms(self):
        """HIP-event time of the write pass of the last run_sides"""
        return self.ctx.L.pgpu_pairing_plan_sides_write_ms(self.h)

    def close(self):
        if self.h:
            self.ctx.L.pgpu_pairing_plan_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class DpPart(C.Structure):
    _fields_ = [("jobs", C.c_void_p), ("n_jobs", C.c_size_t), ("arena", C.c_void_p), ("arena_len", C.c_size_t)]


class JobList:
    """Accumulates DP jobs and their operand bytes (the arena)."""

    def __init__(self):
        self.jobs = []
        self.chunks = []
        self.size = 0

    def _put(self, b: bytes) -> int:
        off = self.size
        self.chunks.append(b)
        self.size += len(b)
        return off

    def add(self, kind, a: bytes, b: bytes, p0=0, p1=0, p2=0, b_tail: bytes = b"",
            a_gen_off=None, b_gen_off=None, tail=None):
        """a/b are operand bytes; with *_gen_off the operand is the slice [off, off+len) of the
        resident genomic instead (a/b then only supply the length)."""
        flags = 0
        if a_gen_off is None:
            a_off = self._put(a)
        else:
            a_off, flags = a_gen_off, flags | JOB_A_GENOMIC
        if b_gen_off is None:
            b_off = self._put(b + b_tail)
        else:
            b_off, flags = b_gen_off, flags | JOB_B_GENOMIC
        self.jobs.append(DpJob(kind, flags, a_off, b_off, len(a), len(b), p0, p1, p2,
                               len(b_tail) if tail is None else tail))
        return len(self.jobs) - 1

    def arrays(self):
        arr = (DpJob * max(len(self.jobs), 1))(*self.jobs)
        return arr, b"".join(self.chunks)


class Plan:
    def __init__(self, ctx: Context, joblist: JobList, index: Index = None):
        self.ctx = ctx
        self.n = len(joblist.jobs)
        self._jobs, self._arena = joblist.arrays()
        self.h = C.c_void_p()
        ctx.check(ctx.L.pgpu_dp_plan_create(ctx.h, index.h if index else None, self._jobs, self.n,
                                            self._arena, len(self._arena), C.byref(self.h)))

    @classmethod
    def from_parts(cls, ctx: Context, joblists, index: Index = None):
        """One plan over several JobLists, each with its own arena (pgpu_dp_plan_create_parts)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.n = sum(len(jl.jobs) for jl in joblists)
        self._keep = []
        parts = (DpPart * max(len(joblists), 1))()
        for k, jl in enumerate(joblists):
            jobs, arena = jl.arrays()
            buf = C.create_string_buffer(arena, len(arena) + 1)
            self._keep += [jobs, buf]
            parts[k] = DpPart(C.cast(jobs, C.c_void_p), len(jl.jobs), C.cast(buf, C.c_void_p), len(arena))
        self.h = C.c_void_p()
        ctx.check(ctx.L.pgpu_dp_plan_create_parts(ctx.h, index.h if index else None, parts, len(joblists), C.byref(self.h)))
        return self

    def launch(self):
        self.ctx.check(self.ctx.L.pgpu_dp_plan_launch(self.ctx.h, self.h))

    def sync(self):
        self.ctx.check(self.ctx.L.pgpu_dp_plan_sync(self.ctx.h, self.h))

    def fetch(self):
        L = self.ctx.L
        nbytes = L.pgpu_dp_plan_string_bytes(self.h)
        res = (DpResult * max(self.n, 1))()
        sbuf = C.create_string_buffer(max(nbytes, 1))
        self.ctx.check(L.pgpu_dp_plan_fetch(self.ctx.h, self.h, res, sbuf, nbytes))
        return res, sbuf.raw

    def results_to_device(self, device_ptr: int, cap: int):
        self.ctx.check(self.ctx.L.pgpu_dp_plan_results_to_device(self.ctx.h, self.h, device_ptr, cap))

    def groups(self):
        L = self.ctx.L
        out = []
        for i in range(L.pgpu_dp_plan_n_groups(self.h)):
            g = GroupInfo()
            L.pgpu_dp_plan_group_info(self.h, i, C.byref(g))
            out.append(dict(name=g.name.decode(), kind=g.kind, jobs=g.jobs, cells=g.cells,
                            algo_bytes=g.algo_bytes, ms=g.ms, t0_ms=g.t0_ms))
        return out

    def close(self):
        if self.h:
            self.ctx.L.pgpu_dp_plan_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


def cstr(buf: bytes, off: int) -> bytes:
    end = buf.index(b"\0", off)
    return buf[off:end]


def decode(kind, r: DpResult, strings: bytes):
    """DpResult -> dict with the field names the oracle wrappers (tests/oracle_lib.py) use."""
    v = r.v
    if r.status != PGPU_OK:
        return dict(status=r.status)
    if kind == ALIGN:
        return dict(status=0, score=v[0], dim=v[1], ea=cstr(strings, r.str[0]),
                    ga=cstr(strings, r.str[1]))
    if kind == GAP:
        return dict(status=0, dim=v[0], factor_cut=v[1], intron_start=v[2], intron_end=v[3],
                    intron_start_on_align=v[4], intron_end_on_align=v[5],
                    ea=cstr(strings, r.str[0]), ga=cstr(strings, r.str[1]))
    if kind == ED:
        return dict(status=0, score=v[0])
    if kind == KBAND:
        return dict(status=0, ok=v[0], edit=v[1], dust=v[2])       # dust: the exon check's two flags (jobs with tail = 1)
    if kind == LCF:
        return dict(status=0, len=v[0], occ1=v[1], occ2=v[2])
    if kind == BORDERS:
        return dict(status=0, ok=v[0], off_p=v[1], off_t1=v[2], off_t2=v[3], ed=v[4])
    if kind == AFFIX:
        return dict(status=0, valid=v[0], ecut=v[1], gcut=v[2])
    raise ValueError(kind)


def run_jobs(ctx: Context, joblist: JobList, index: Index = None):
    """create + launch + sync + fetch + destroy; returns a list of decoded dicts."""
    plan = Plan(ctx, joblist, index)
    try:
        plan.launch()
        plan.sync()
        res, strings = plan.fetch()
        return [decode(joblist.jobs[i].kind, res[i], strings) for i in range(plan.n)]
    finally:
        plan.close()
