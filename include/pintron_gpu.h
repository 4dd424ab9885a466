/*
 * pintron_gpu.h -- C-ABI of the MI355X (gfx950) est-fact accelerator library, libpintron_gpu.so.
 *
 * This is the drop-in boundary for PIntron's est-fact hot path: plain C, pointers and sizes only.
 * Each entry point names the reference routine(s) it replaces (paths relative to the AlgoLab/PIntron
 * tree).  The library has NO CPU fallback: every call fails with PGPU_EDEVICE when no gfx950
 * device is usable.
 *
 * Threading: a pgpu_ctx owns one HIP stream; calls on one context must be serialised by the
 * caller, different contexts are independent.  All functions return 0 (PGPU_OK) or a negative
 * errno-style code and never abort.
 */
#ifndef PINTRON_GPU_H
#define PINTRON_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGPU_OK       0
#define PGPU_EDEVICE (-5)    /* HIP runtime error / no device (EIO) */
#define PGPU_ENOMEM  (-12)
#define PGPU_EINVAL  (-22)
#define PGPU_ENOSPC  (-28)   /* caller's output buffer too small */
#define PGPU_ERANGE  (-34)   /* a job exceeds the supported dimensions (per-job status) */
#define PGPU_ENOSYS  (-38)   /* entry point not implemented in this build */

typedef struct pgpu_ctx pgpu_ctx;
typedef struct pgpu_index pgpu_index;
typedef struct pgpu_dp_plan pgpu_dp_plan;

/* ------------------------------------------------------------------------------------------ */
/* context                                                                                    */
/* ------------------------------------------------------------------------------------------ */
int pgpu_init(int device, pgpu_ctx** ctx);
int pgpu_destroy(pgpu_ctx* ctx);
/* human-readable text of the last error on this context (never NULL) */
const char* pgpu_last_error(const pgpu_ctx* ctx);
/* ABI version of the loaded library */
int pgpu_abi_version(void);
/* HIP-event timing of every kernel group of the plans created afterwards (off by default; the
 * measurement hooks below return 0 without it) */
int pgpu_set_timing(pgpu_ctx* ctx, int enabled);
/* NUMA node of the host the context's GPU hangs off (its PCI device's numa_node), or -1 when the
 * platform does not say.  The est-fact host binds its threads to that node: on a two-socket host
 * that alone is worth 10-14 % (the per-EST logic is memory-latency bound and the batches cross
 * PCIe on that socket). */
int pgpu_device_numa_node(pgpu_ctx* ctx);
/* Profiler ranges (roctx): the library wraps the kernel groups of every plan ("dp_batch", "lcf",
 * "pairings", "meg", "index build") and the host program its phases ("est-fact step", "prefetch chunk k")
 * so that `rocprofv3 --marker-trace` shows them.  The reference has five wall-clock timers
 * (src/main-est-fact.c:95-99) and nothing per routine; SURVEY.md section 5 asks for both.  The roctx library is
 * loaded on first use and only when PGPU_MARKERS=1 or a rocprofiler tool is in the process; otherwise the
 * calls are two loads and a branch. */
void pgpu_range_push(const char* name);
void pgpu_range_pop(void);
/* identity of the loaded library: compiler, target and an FNV-1a hash of the code object bundle's build
 * stamp (__DATE__ __TIME__ + the compiler version) -- what smoke() prints so that a record can tell which
 * binary ran */
const char* pgpu_build_info(void);

/* ------------------------------------------------------------------------------------------ */
/* genomic index -- replaces lst_stree_new (stree_src/lst_stree.c:816) + preprocess_text /     */
/* stree_preprocess (src/aug_suffix_tree.c:68,247), called at src/main-est-fact.c:224-239.    */
/* The genomic sequence (after Ntails_removal) is copied to HBM once, with its suffix array.  */
/* ------------------------------------------------------------------------------------------ */
int pgpu_index_build(pgpu_ctx* ctx, const char* genomic, size_t len, pgpu_index** idx);
int pgpu_index_destroy(pgpu_ctx* ctx, pgpu_index* idx);
/* The index depends on the genomic sequence alone, and a gene is processed many times (re-runs of
 * the pipeline, parameter studies): save writes suffix array, LCP array and k-mer table to a file,
 * load brings them back into HBM without the construction.  load returns PGPU_EINVAL when the file
 * is missing, damaged or was made for another sequence (length + hash are checked) -- the caller
 * then builds.   */
int pgpu_index_save(pgpu_ctx* ctx, const pgpu_index* idx, const char* genomic, const char* path);
int pgpu_index_load(pgpu_ctx* ctx, const char* path, const char* genomic, size_t len, pgpu_index** idx);
/* copies the suffix array (len entries) back to the host; for tests and diagnostics */
int pgpu_index_suffix_array(pgpu_ctx* ctx, const pgpu_index* idx, uint32_t* sa_out, size_t cap);

/* ------------------------------------------------------------------------------------------ */
/* exact occurrences -- the other thing a suffix tree of the genomic is for: where does this   */
/* string occur, byte for byte, inside this stretch of the sequence.  Replaces the strstr()    */
/* loop of search_small_exon (src/factorization-refinement.c:781-834), which scans a whole     */
/* intron for every (offstart, offend) pair.                                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t pat_off;      /* pattern bytes at patterns + pat_off                          */
  uint32_t pat_len;
  uint32_t reserved;     /* must be 0                                                    */
  uint32_t lo, hi;       /* only occurrences t with lo <= t and t + pat_len <= hi count  */
} pgpu_find_query;       /* 24 bytes */

/* One batched call, synchronous: it returns after the answers have been downloaded.
 *  - An occurrence is equality of pat_len BYTES, exactly what strstr / memcmp see in the reference
 *    (the strstr of src/factorization-refinement.c:794-795): case-sensitive, and 'N' is a letter like any
 *    other -- NOT a wildcard here, unlike PGPU_DP_ALIGN / GAP / LCF.  Overlapping occurrences all count
 *    (the reference goes on one byte behind each hit, :829).
 *  - out_first[q]..out_first[q+1] delimits the answers of query q (n_queries + 1 entries); within a query the
 *    positions are ascending (the order in which the strstr loop meets them); *n_out is the total (n_out may be
 *    NULL).  When out_cap is too small the call returns PGPU_ENOSPC, has still filled out_first and *n_out, and
 *    has written nothing to out.  out == NULL with out_cap == 0 asks for the counts alone (PGPU_OK when there is
 *    no occurrence at all).
 *  - hi is clamped to the length of the sequence.  lo > hi, pat_off + pat_len > patterns_len or reserved != 0 in
 *    any query is PGPU_EINVAL for the whole call.  pat_len == 0, a pattern longer than its window, or a window
 *    that lies behind the end of the sequence gives an empty answer, not an error.  n_queries == 0 is PGPU_OK
 *    with *n_out = 0 and out_first[0] = 0.
 *  - idx may come from pgpu_index_build or from pgpu_index_load. */
int pgpu_index_find(pgpu_ctx* ctx, const pgpu_index* idx,
                    const char* patterns, size_t patterns_len,
                    const pgpu_find_query* queries, size_t n_queries,
                    uint32_t* out, size_t out_cap, uint64_t* out_first, size_t* n_out);
/* HIP-event time of the kernels of the calling thread's last pgpu_index_find on a context with timing on
 * (pgpu_set_timing): k = 0 count + scan, 1 fill; 0 without timing or when the stage did not run */
double pgpu_index_find_kernel_ms(int k);

/* ------------------------------------------------------------------------------------------ */
/* intron classes and the small-exon search -- what search_small_exon                          */
/* (src/factorization-refinement.c:641-871) does with every occurrence: it classifies the two  */
/* introns the occurrence would create (_classify_intron, :612-629, which is                   */
/* classify_genomic_intron_start_end, src/classify-intron.c:95-229) and keeps the longest      */
/* small exon whose two introns are both classified (:772-834).  Both are answered from        */
/* classification tables of the index (the four 5' splice-site scores of every start, the      */
/* branch-point verdict of every end), built on the device at the first of these calls on an   */
/* index, built or loaded, and kept until pgpu_index_destroy; the index file does not hold     */
/* them.  All three calls are synchronous like pgpu_index_find.                                */
/* ------------------------------------------------------------------------------------------ */
typedef struct { uint32_t start, end; } pgpu_intron;      /* both inclusive, as the reference's */

/* classify_genomic_intron_start_end (src/classify-intron.c:95-229), the class alone: out_type[i] = 0 U12, 1 U2,
 * 2 not classified, for the intron genomic[start .. end].  Identical to the reference wherever the reference is
 * defined; elsewhere: an intron is cut at the end of the sequence (end at or behind the last byte), end < start
 * or start at or behind the end is the empty intron, a motif with a byte outside ACGTNacgtn scores -1.0.  Lower
 * case counts like upper case and N like A, as in the reference.  No per-query error; n == 0 is PGPU_OK. */
int pgpu_index_classify(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_intron* introns, size_t n,
                        uint8_t* out_type);
/* diagnostics, like pgpu_index_suffix_array: the table of 5' matrix k (0 GTAG-U12, 1 ATAC-U12, 2 GTAG-U2,
 * 3 GCAG-U2), len + 1 doubles: what GetScoreOf5Prime*BySS (src/classify-intron.c:231-330) returns for every start,
 * bit for bit.  PGPU_ENOSPC when cap < len + 1. */
int pgpu_index_score5(pgpu_ctx* ctx, const pgpu_index* idx, int k, double* out, size_t cap);

/* One query = one execution of the block at src/factorization-refinement.c:760-834: what is left of
 * search_small_exon when the edit distances and common factors in front of it (PGPU_DP_ED / PGPU_DP_LCF) are known. */
#define PGPU_SEXON_MAX_ELEN 64
typedef struct {
  uint64_t e_off;            /* efact = ests + e_off, elen bytes (the reference's efact, :761-763)          */
  uint32_t elen;
  uint32_t allgstart, allglen;   /* allgfact = genomic[allgstart .. allgstart + allglen)  (:766-768)        */
  uint32_t f1slen, f2plen;   /* perfect-border lengths (:708-737)                                           */
  uint32_t min_intron_len;   /* MAX(4, config->min_intron_length) (:742); < 4 is PGPU_EINVAL                */
  uint32_t reserved;         /* must be 0                                                                   */
  /* 4 bytes of padding follow (the struct is aligned to its uint64_t): their content is ignored            */
} pgpu_sexon_query;          /* 40 bytes */
typedef struct {
  int32_t  status;           /* PGPU_OK, or PGPU_ERANGE: elen > PGPU_SEXON_MAX_ELEN                         */
  uint32_t len;              /* max_sexon_len (:772); 0 = none found, every field below is 0 then           */
  uint32_t offstart, offend; /* of the winner                                                               */
  uint32_t gpos;             /* genomic position of the small exon's first base (= gcut1_2, :822)           */
  uint32_t i1type, i2type;   /* classes of the two introns of the winner (0 U12, 1 U2)                      */
  uint32_t pad;              /* 0 */
} pgpu_sexon_result;         /* 32 bytes */

/*  - The four gates of :743-758 (f1slen < 6, f2plen < 6, allglen < 2 * min_intron_len + 6, elen < 6) give len = 0,
 *    not an error: the reference ends the search there.  allgstart + allglen > len of the sequence,
 *    e_off + elen > ests_len, reserved != 0 or min_intron_len < 4 in any query is PGPU_EINVAL for the whole call.
 *  - The loop bounds max_offstart and max_offend are those of :776-785.  For (offstart, offend) the pattern is
 *    efact[offstart .. elen - offend); an occurrence counts when it starts at or behind
 *    allgstart + offstart + min_intron_len and ends at or before allgstart + allglen - offend - min_intron_len.
 *    Occurrences are byte equality as in pgpu_index_find: case-sensitive, N a letter, overlapping ones all count.
 *  - The introns of an occurrence occ are i1 = [allgstart + offstart, occ - 1] and
 *    i2 = [occ + pattern length, allgstart + allglen - offend - 1]; a candidate needs both classes != 2 (:805-809).
 *  - The winner.  The reference replaces its best candidate on strictly greater length only (:816), so among the
 *    candidates of maximal length the FIRST in loop order wins: the smallest offstart, then the smallest
 *    occurrence (offend follows from the length). */
int pgpu_index_small_exons(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                           const pgpu_sexon_query* q, size_t n, pgpu_sexon_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_small_exons on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_small_exons_kernel_ms(void);

/* ------------------------------------------------------------------------------------------ */
/* intron borders -- what refine_intron (src/refine-intron.c:47-265) does with the 3-state gap  */
/* alignment of an intron (PGPU_DP_GAP, which stays a job of the caller): the canonical-site    */
/* searches on the gapped rows (Find_*, :892-990, :1852-1972), the four shift heuristics with   */
/* their edit distances (Shift_*, :992-1850), the Burset fallback (Try_Burset_after_match,      */
/* :267-344) and the tests that accept or refuse the result (:123-155, :245-257).  One query =  */
/* one intron; the call is synchronous and batched like pgpu_index_small_exons.                 */
/* ------------------------------------------------------------------------------------------ */
typedef struct { int32_t EST_start, EST_end, GEN_start, GEN_end; } pgpu_factor;   /* the reference's _factor, inclusive; 16 bytes */

#define PGPU_REFINE_MAX_DIM 1024      /* alignment columns per query; beyond: PGPU_ERANGE for that query */
#define PGPU_REFINE_MAX_ED   256      /* bytes of one operand of an edit distance; beyond: PGPU_ERANGE for that query.
                                         The default configuration's windows (30 + gap + 30 against 30 + 70 + 70 + 30)
                                         cannot make a longer one: an operand is a piece of one window plus at most
                                         16 bytes of the rows */
#define PGPU_REFINE_FIRST_INTRON 1u   /* flags bit 0 */

typedef struct {
  uint64_t est_off;  uint32_t est_len;        /* est_info->EST_seq = ests + est_off, est_len bytes                          */
  uint32_t flags;                              /* bit 0: first_intron; other bits must be 0                                  */
  uint64_t rows_off; uint32_t dim;             /* EST_gap_alignment = rows + rows_off, GEN_gap_alignment = rows + rows_off + dim,
                                                  dim bytes each (no terminator needed)                                      */
  int32_t  factor_cut, intron_start, intron_end, intron_start_on_align, intron_end_on_align;   /* v[1..5] of the PGPU_DP_GAP result */
  pgpu_factor donor, acceptor;                 /* the two exons as they are when the alignment's windows are cut             */
  int32_t  suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen, min_intron_length;
  /* offsets: est_off 0, est_len 8, flags 12, rows_off 16, dim 24, factor_cut 28 .. intron_end_on_align 44, donor 48,
   * acceptor 64, suffpref_length_on_est 80 .. min_intron_length 92: no padding anywhere */
} pgpu_refine_query;         /* 96 bytes */

typedef struct {
  int32_t status;                  /* PGPU_OK or PGPU_ERANGE (then refined = 0, path = 0, the factors unchanged)            */
  int32_t refined;                 /* refine_intron's return value                                                           */
  int32_t path;                    /* which branch decided, see below                                                        */
  int32_t pad;                     /* 0 */
  pgpu_factor donor, acceptor;     /* as refine_intron leaves them (unchanged when refined == 0)                             */
} pgpu_refine_result;        /* 48 bytes */

/*  - path: 0 donor attached, first intron (:127-135, refined 1); 1 donor attached, not the first intron (:136-140,
 *    refined 0); 2 intron too small (:143, 0); 3 a border shifted by more than 20 (:151, 0); 4 already canonical (:189, 1);
 *    5 Shift_right_to_left_1; 6 Shift_left_to_right_1; 7 Shift_right_to_left_2; 8 Shift_left_to_right_2; 9 Burset.  For
 *    5 - 9 refined is 0 when the test of :245 refuses the borders.
 *  - The call derives donor_suffix_left_on_est / _on_gen and deleted_intron_dim from the factors and the three lengths
 *    (:55-64, :110) and from there does what the reference does, quirks included: the comparisons with "AG", "GT", "GC"
 *    are case-sensitive, the Burset lookup is not; `error` and `edit_prev` of the two _1 routines are unsigned and wrap;
 *    the mismatch count taken off the extended distances is the one of the GENOMIC eight-column piece; two cycles.
 *    The edit distances are PGPU_DP_ED's (Levenshtein, N no wildcard).  All distances one Shift_* routine can ask for
 *    (at most six) are computed together once its two cycles are known; an operand longer than PGPU_REFINE_MAX_ED among
 *    them refuses the query.
 *  - Where the reference's scans leave their strings: a row byte outside [0, dim) reads as 0; a 0 inside a row ends
 *    it (strlen), and in an empty genomic row Find_AG_after_on_the_right finds nothing; a byte of the EST outside
 *    [0, est_len) and a byte of the genomic sequence outside [0, its length) read as 0, and both strings end at their
 *    terminator (real_substring stops there).
 *  - PGPU_EINVAL for the whole call, in any query: est_off + est_len > ests_len or rows_off + 2 * dim > rows_len; an
 *    unknown flag bit; dim == 0; donor.EST_end >= acceptor.EST_start or donor.GEN_end >= acceptor.GEN_start (the
 *    my_asserts of :52-53); a coordinate that is no offset into what it indexes: a factor's EST_* outside
 *    [-1, est_len], GEN_* outside [-1, length of the sequence], one of the five alignment values outside [0, dim], a
 *    suffpref length that is negative or above 2^24 (min_intron_length is only compared: any value).  n == 0 is
 *    PGPU_OK.  idx may be built or loaded. */
int pgpu_index_refine_introns(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                              const char* rows, size_t rows_len,
                              const pgpu_refine_query* q, size_t n, pgpu_refine_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_refine_introns on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_refine_introns_kernel_ms(void);

/* All of refine_intron, chained per EST: the loop of src/est-factorizations.c:446-490 over one factorization, with the
 * window cutting (src/refine-intron.c:55-116), the 3-state gap alignment (compute_gap_alignment, :560-890) and the border
 * decision above done on the device for one intron after the other.  Each call of the loop changes its acceptor, and that
 * acceptor is the donor of the next call, so the windows of intron k + 1 exist only when intron k is settled: nothing of an
 * intron leaves the device between its windows and its verdict.  One query = one factorization; the call is synchronous and
 * batched like pgpu_index_refine_introns. */
#define PGPU_CHAIN_MAX_EST_WINDOW 192   /* bytes of the EST window of one intron; beyond: PGPU_ERANGE for that chain            */
#define PGPU_CHAIN_MAX_GEN_WINDOW 320   /* bytes of its genomic window.  The default configuration (30 + gap + 30 against
                                           30 + 70 + 70 + 30) fits with an unaligned EST gap of up to 132 bytes               */
typedef struct {
  uint64_t est_off; uint32_t est_len;     /* est_info->EST_seq = ests + est_off, est_len bytes (at most 2^31 - 1)                */
  uint32_t first_exon, n_exons;           /* the factorization = exons[first_exon .. first_exon + n_exons)                       */
  uint32_t reserved;                      /* must be 0                                                                           */
  int32_t  suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen, min_intron_length;
  /* offsets: est_off 0, est_len 8, first_exon 12, n_exons 16, reserved 20, suffpref_length_on_est 24 .. min_intron_length 36:
   * no padding anywhere */
} pgpu_chain_query;          /* 40 bytes */

typedef struct {
  int32_t  status;        /* PGPU_OK, or PGPU_ERANGE: an intron did not fit the caps                                             */
  uint32_t done;          /* introns settled (n_exons - 1 on PGPU_OK); on PGPU_ERANGE the index of the one refused: out_exons
                             holds the chain as it stood BEFORE that intron and the caller goes on from there on its own path  */
  uint32_t dropped_first; /* 1 when the rule of est-factorizations.c:476-485 removed the first exon (first and second exon
                             begin at the same EST position; only when the whole chain was done): the exon stays in out_exons,
                             the caller skips it                                                                                */
  uint32_t pad;           /* 0 */
} pgpu_chain_result;         /* 16 bytes: status 0, done 4, dropped_first 8, pad 12 */

/*  - out_exons (n_exons_total entries) is parallel to exons: same indices; exons no query names are copied unchanged.
 *    out_steps (n_exons_total bytes) is parallel too: for the exon at place i >= 1 of a chain, what pgpu_refine_result holds
 *    for the intron in front of it -- path in bits 0-3, refined in bit 7; 0 for a chain's first exon and for introns never
 *    reached.
 *  - Per intron, in chain order, the call does refine_intron(config, gen, est, &exon[i], &exon[i + 1], i == 0) on the exons
 *    as they are at that moment: the windows are the real_substring pieces of :55-116 with the clamping of
 *    ef_gap_window_build (a negative index shortens the piece, a piece ends at the terminator -- the end of the EST, of the
 *    sequence, or a 0 byte -- and a negative length is empty); the alignment is PGPU_DP_GAP's, bit for bit (the same rows,
 *    the same five values); the decision is pgpu_index_refine_introns', with every quirk listed there.
 *  - The reference overruns its own sequence_on_est block when the EST has an unaligned gap between the two exons (:84-87:
 *    the block is sized for the donor's suffix and the acceptor's prefix, the gap is appended as well).  There the entry is
 *    defined by the restatement: the strings as ef_gap_window_build makes them.
 *  - n_exons == 1 is a chain with nothing to do (PGPU_OK, done 0).  n == 0 is PGPU_OK (out_exons = exons, out_steps = 0).
 *  - Caps: a window longer than PGPU_CHAIN_MAX_EST_WINDOW / _GEN_WINDOW, or an edit-distance operand longer than
 *    PGPU_REFINE_MAX_ED, ends THAT chain with PGPU_ERANGE as described at `done`; it never affects another chain.  (The
 *    alignment of two windows within the caps has at most 512 columns: PGPU_REFINE_MAX_DIM cannot refuse.)
 *  - PGPU_EINVAL for the whole call: n_exons == 0; first_exon + n_exons > n_exons_total or est_off + est_len > ests_len;
 *    est_len > 2^31 - 1; reserved != 0; two chains share an exon; a factor coordinate outside what
 *    pgpu_index_refine_introns accepts (EST_* outside [-1, est_len], GEN_* outside [-1, length of the sequence]); a suffpref
 *    length outside [0, 2^24]; for some adjacent pair exon[i].EST_end >= exon[i + 1].EST_start or exon[i].GEN_end >=
 *    exon[i + 1].GEN_start (the my_asserts of :52-53).  The last can be checked up front because it concerns fields no
 *    earlier step writes: refining the pair (i - 1, i) changes EST_start and GEN_start of exon i alone, and EST_end and
 *    GEN_end of exon i and the starts of exon i + 1 are written by the refinement of the pair (i, i + 1) itself.
 *  - idx may be built or loaded. */
int pgpu_index_refine_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                             const pgpu_factor* exons, size_t n_exons_total,
                             const pgpu_chain_query* q, size_t n,
                             pgpu_factor* out_exons, uint8_t* out_steps, pgpu_chain_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_refine_chains on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_refine_chains_kernel_ms(void);

/* A candidate factorization's cleaning steps, chained: what get_EST_factorizations (src/est-factorizations.c:212-244) does
 * to one candidate before refine_intron sees it -- check_for_not_source_sink_factorization, check_exon_start_end,
 * handle_endpoints, clean_external_exons, clean_low_complexity_exons_2, clean_noisy_exons and check_est_coverage -- with
 * the two end-exon alignments, their trimming, the dust scores and the banded edit distances done on the device for one
 * step after the other.  One query = one candidate; the call is synchronous and batched like pgpu_index_refine_chains.
 * add_if_not_exists compares candidates with each other and stays with the caller. */
#define PGPU_CLEAN_MAX_EXONS      64    /* exons of one factorization; beyond: PGPU_ERANGE for that query   */
#define PGPU_CLEAN_MAX_END_EXON 4096    /* bytes of an end exon on the EST and on the genomic sequence      */
typedef struct {
  uint64_t est_off; uint32_t est_len;   /* EST_seq = ests + est_off, est_len bytes, 1 .. 2^31 - 1           */
  uint32_t first_exon, n_exons;         /* the candidate = exons[first_exon .. first_exon + n_exons)        */
  uint32_t reserved;                    /* 0 */
  double   complexity_threshold;        /* config->complexity_threshold */
} pgpu_clean_query;                     /* 32 bytes: 0, 8, 12, 16, 20, 24; no padding */
typedef struct {
  int32_t  status;                      /* PGPU_OK or PGPU_ERANGE */
  uint32_t verdict;                     /* 0 kept; the step that rejected: 1 source-sink, 2 start/end order, 3 emptied by
                                           handle_endpoints, 4 by clean_external_exons, 5 by clean_low_complexity_exons_2,
                                           6 by clean_noisy_exons, 7 check_est_coverage */
  uint32_t first_kept, n_kept;          /* the list as it stood when the verdict fell (verdicts 0 and 7), as indices into
                                           the query's exons; 0, 0 otherwise */
} pgpu_clean_result;                    /* 16 bytes */

/*  - out_exons (n_exons_total entries) and out_marks (n_exons_total bytes) are parallel to exons: same indices; exons no
 *    query names are copied, with mark 0.  Only the first EST_start / GEN_start and the last EST_end / GEN_end of the run
 *    [first_kept, first_kept + n_kept) of a query with verdict 0 or 7 can differ from the input; every other exon is a copy.
 *    out_marks: bit 0 dropped by handle_endpoints, bit 1 dropped by clean_external_exons, bit 2 dust(genomic) > threshold,
 *    bit 3 dust(EST) > threshold, bit 4 the K-band verdict was false.  A step that never ran leaves its bits 0.
 *  - The steps, in order, each on the list as the one before left it (lines of src/est-factorizations.c):
 *    1. :2111-2125 (one exon whose EST_start lies outside [0, est_len): verdict 1), then :1989-2019 (an exon with
 *       start > end on either string, or a start in front of the end of the exon before it: verdict 2).
 *    2. handle_endpoints (:2127-2301).  Each alignment is PGPU_DP_ALIGN's, bit for bit: a = the exon on the EST, b = the
 *       exon on the genomic sequence, N a wildcard.  The head is walked from the left until "more than 5 matches", tested
 *       one column late: an alignment of exactly six matching columns drops the exon, seven keep it; the exon then begins
 *       where that run of matches begins.  The tail likewise from the right with "more than 10", and it ends where that
 *       run ends; its gap-closing loop (:2241-2281) then rewrites the rows as it goes, and a byte behind a row reads 0.  The
 *       tail is dropped only when its new GEN_end lies in front of its GEN_start: a walk that reaches the first column
 *       without stopping keeps a tail whose first column matches (eleven matching columns and nothing else: kept whole)
 *       and drops one whose first column does not (that column, then ten matches: dropped; then eleven: kept).  With one
 *       exon the tail step aligns the head as already trimmed.
 *    3. clean_external_exons (:1706-1825): an end exon shorter than 10 on the genomic sequence is dropped; one shorter than
 *       20 stays only with its splice sites (G, then T or C behind the head and behind the exon before the tail; A, G in
 *       front of the tail and of the exon behind the head; compared case-insensitively, a genomic byte outside the
 *       sequence reads as 0, and an exon without that neighbour is dropped) and an edit distance of 0 between its two
 *       strings.  The distance is only tested `> 0`, which is exactly "the two real_substring pieces differ as byte
 *       strings", no wildcard: no DP is run for it.
 *    4. clean_low_complexity_exons_2 (:1667-1704): PGPU_DP_KBAND's `tail = 1` dust flags for every exon, then
 *       update_with_subfact_with_best_coverage (:1900-1987) over the flagged ones: the run of unflagged exons with the
 *       largest EST_end - EST_start + 1 stays; a strictly larger cover wins, so the first of equals does.
 *    5. clean_noisy_exons (:1842-1898) with only_internals = false: the bound of :1828-1839 in FP64 from the genomic length,
 *       K_band_edit_distance as PGPU_DP_KBAND has it, early exits included; then the same best-run rule.
 *    6. check_est_coverage (:2303-2321): (double) cover / (double) est_len >= (double) 0.35f, else verdict 7.
 *  - Caps refuse only the query that reaches them: its result is PGPU_ERANGE with verdict, first_kept and n_kept 0, its exons
 *    are copied unchanged and their marks are 0.  More than PGPU_CLEAN_MAX_EXONS exons (tested before step 1); an end exon,
 *    as it is when it is aligned, longer than PGPU_CLEAN_MAX_END_EXON on either string; an end-exon alignment the plan
 *    builder would send neither to lev_wave<ALIGN> (at most 64 EST bytes) nor to an align_band job settled inside the band
 *    (65 .. 4096 EST bytes, lengths within 31 of each other, score <= 31); an exon in the list at step 5 whose bound exceeds
 *    31, i.e. a genomic length above 1 033.  A query an earlier step rejects never reaches a later cap.
 *  - PGPU_EINVAL for the whole call: a null pointer (no message); n_exons == 0; first_exon + n_exons > n_exons_total or
 *    est_off + est_len > ests_len; est_len == 0 or > 2^31 - 1; reserved != 0; two queries share an exon; a factor coordinate
 *    outside what pgpu_index_refine_introns accepts; for a query that passes the two checks of step 1 (whatever its number of
 *    exons): a first exon with EST_start < 0 or GEN_start < 0, or a last exon with EST_end >= est_len or GEN_end >= the length of
 *    the sequence (the my_asserts of :2140-2141 and :2199-2200, which the reference's build compiles out).
 *  - n == 0 is PGPU_OK (out_exons = exons, out_marks = 0).  idx may be built or loaded. */
int pgpu_index_clean_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                            const pgpu_factor* exons, size_t n_exons_total, const pgpu_clean_query* q, size_t n,
                            pgpu_factor* out_exons, uint8_t* out_marks, pgpu_clean_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_clean_chains on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_clean_chains_kernel_ms(void);

/* check_gap_errors of a factorization, chained: FILTER 4 of get_EST_factorizations (src/est-factorizations.c:416-433, the
 * routine at :1462-1545), the step between the cleaning steps above and the refinement loop of pgpu_index_refine_chains --
 * for every unaligned EST gap between two exons a border refinement (refine_borders, src/refine.c:85-192) against the
 * intron, the four exon ends that face the gap moved, the distances summed against the threshold of :1465, and the exons
 * whose genomic gap is at most 3 merged.  One query = one factorization; the call is synchronous and batched like
 * pgpu_index_clean_chains, and its exon arrays have the same shape.  FILTER 1 and FILTER 3 compare candidates with each
 * other and stay with the caller, as add_if_not_exists does. */
#define PGPU_GAPS_MAX_EXONS    64   /* exons of one factorization; beyond: PGPU_ERANGE for that query            */
#define PGPU_GAPS_MAX_EST_GAP  64   /* bytes of one EST gap (the BORDERS pattern: one row per lane); beyond: same */
#define PGPU_GAPS_MAX_ERRORS   20   /* threshold_ed of :1465 */
typedef struct {
  uint64_t est_off; uint32_t est_len;   /* EST_seq = ests + est_off, est_len bytes, 1 .. 2^31 - 1 */
  uint32_t first_exon, n_exons;         /* the factorization = exons[first_exon .. first_exon + n_exons) */
  uint32_t reserved;                    /* 0 */
} pgpu_gaps_query;                      /* 24 bytes: 0, 8, 12, 16, 20; no padding */
typedef struct {
  int32_t  status;       /* PGPU_OK or PGPU_ERANGE */
  uint32_t verdict;      /* 0 kept; 1 dropped: the distances of its gaps sum to more than 20 (:1517) */
  uint32_t total_edit;   /* tot_out_edit_distance */
  uint32_t n_kept;       /* exons left after the merging loop (verdict 0); 0 otherwise */
} pgpu_gaps_result;      /* 16 bytes */

/*  - The border loop (:1475-1514), for each adjacent pair (d, a) in order: gapP = a.EST_start - d.EST_end - 1 and
 *    gapT = a.GEN_start - d.GEN_end - 1, both taken from the input -- a gap writes only the four ends that face it, so the
 *    strings of every gap are the input's.  When gapP > 0: general_refine_borders(p, gapP, 0, gapP, t, gapT, max_errs =
 *    gapP) with p = the EST gap and t = the whole genomic gap, read from the resident sequence, with `tail = 0`: the
 *    reference works on NUL-terminated copies (real_substring, :1489-1490), so getBursetFrequency_adaptor sees a terminator
 *    behind t, not the acceptor exon.  The result is PGPU_DP_BORDERS's, bit for bit: plain byte equality with N no
 *    wildcard, t_win = min(2 gapP, gapT), the first cut with the smallest total, ties broken by a strictly larger Burset
 *    frequency.  Then, as :1502-1506: d.EST_end += off_p; a.EST_start = d.EST_end + 1; d.GEN_end += off_t1;
 *    a.GEN_start -= gapT - off_t2.
 *  - refine_borders cannot refuse here: its total is at most len_p (every row minimum is at most the row's first column)
 *    and max_errs = len_p, so the `ok == false` branch of :1508 is dead.
 *  - The verdict: a total above PGPU_GAPS_MAX_ERRORS is verdict 1 (:1517).
 *  - The merging loop (:1522-1542), on verdict 0, with a running donor: an exon whose GEN_start - donor.GEN_end - 1 <= 3
 *    (negative included) gives its EST_end and GEN_end to the donor and is removed; any other exon becomes the donor.
 *  - out_exons (n_exons_total entries) and out_steps (n_exons_total bytes) are parallel to exons: same indices; exons no
 *    query names are copied, with step 0.  out_steps[i] for the exon at place i >= 1 of a query: bits 0-6 are 0 when the EST
 *    gap in front of it was empty, else 1 + that gap's edit distance (1 .. 65); bit 7: the exon was merged into the one
 *    before it.  A merged exon's out_exons entry holds the exon as the border loop left it, the donor's entry holds the
 *    merged ends.  On verdict 1 out_exons is what the border loop left, and no bit 7 is set.
 *  - Caps refuse only the query that meets them: its result is PGPU_ERANGE with verdict, total_edit and n_kept 0, its exons
 *    are copied unchanged and their steps are 0.  More than PGPU_GAPS_MAX_EXONS exons; an EST gap longer than
 *    PGPU_GAPS_MAX_EST_GAP.  The genomic gap has no cap of its own: only its first and last t_win <= 128 bytes are read.
 *  - PGPU_EINVAL for the whole call: a null pointer (no message); n_exons == 0; first_exon + n_exons > n_exons_total or
 *    est_off + est_len > ests_len; est_len == 0 or > 2^31 - 1; reserved != 0; two queries share an exon; a factor coordinate
 *    outside what pgpu_index_refine_introns accepts; for some adjacent pair exon[i].EST_end >= exon[i + 1].EST_start or
 *    exon[i].GEN_end >= exon[i + 1].GEN_start; for some adjacent pair gapP > gapT (the FATAL of :1485, where the reference
 *    ends the program).  All of these are properties of the input and are checked up front; with them both pieces of
 *    every gap lie inside their strings.  A 0 byte inside the EST is a letter like any other.
 *  - n == 0 is PGPU_OK (out_exons = exons, out_steps = 0); n_exons == 1 is verdict 0, n_kept 1.  idx may be built or
 *    loaded. */
int pgpu_index_gap_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                          const pgpu_factor* exons, size_t n_exons_total, const pgpu_gaps_query* q, size_t n,
                          pgpu_factor* out_exons, uint8_t* out_steps, pgpu_gaps_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_gap_chains on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_gap_chains_kernel_ms(void);

/* What est-fact does to a factorization directly behind the refinement loop, chained: the end of get_EST_factorizations
 * (correct_composition_tail and detect_polyA_signal, src/detect-polya.c:42-166, called at src/est-factorizations.c:573-585)
 * and the first steps of refine_EST_factorizations that concern one factorization alone (src/factorization-refinement.c:
 * remove_invalid_factorizations :120-165, recover_lost_prefixes_and_suffixes :1177-1266, remove_false_small_exons
 * :959-1125).  One query = one factorization; the call is synchronous and batched like pgpu_index_gap_chains, and its exon
 * arrays have the same shape.  remove_duplicated_factorizations compares factorizations with each other and stays with the
 * caller.  Nothing in the library calls this entry yet. */
#define PGPU_TAIL_MAX_EXONS         64   /* exons of one factorization; beyond: PGPU_ERANGE for that query */
#define PGPU_TAIL_MAX_AFFIX        256   /* EST bytes of a lost prefix / suffix window whose DP has to run; beyond: same */
#define PGPU_TAIL_MAX_SMALL_WINDOW 128   /* EST bytes of the BORDERS pattern of a small-exon analysis; beyond: same */
#define PGPU_TAIL_MAX_SMALL_GEN    256   /* genomic bytes of an analysed exon whose edit distance has to run; beyond: same */
#define PGPU_TAIL_WIDE_MAX_AFFIX  1024   /* the same window in pgpu_index_tail_chains_wide: sixteen rows of the DP per lane */
#define PGPU_TAIL_UB_MED_EXON      100   /* _UB_MED_EXON_: a longer exon (on the EST) is not analysed in step 5 */
#define PGPU_TAIL_AFFIXES_LENGTH     5   /* _AFFIXES_LENGTH_: what step 5 takes of the two neighbours */
typedef struct {
  uint64_t est_off; uint32_t est_len;   /* the WORKING sequence (polyA/T masked) = ests + est_off, est_len bytes, 1 .. 2^31 - 1:
                                           steps 4 and 5 */
  uint32_t first_exon, n_exons;         /* the factorization = exons[first_exon .. first_exon + n_exons) */
  uint32_t reserved;                    /* 0 */
  uint64_t orig_off;                    /* the ORIGINAL sequence = ests + orig_off, est_len bytes too: steps 1 and 2; may
                                           equal est_off */
} pgpu_tail_query;                      /* 32 bytes: 0, 8, 12, 16, 20, 24; no padding */
typedef struct {
  int32_t  status;       /* PGPU_OK or PGPU_ERANGE */
  uint8_t  verdict;      /* 0 kept; 1 removed by remove_invalid_factorizations */
  uint8_t  polyA;        /* detect_polyA_signal's return value */
  uint8_t  polyadenil;   /* its *polyadenil */
  uint8_t  recovered;    /* bit 0: a prefix was recovered, bit 1: a suffix */
  uint32_t n_kept;       /* exons left after step 5 (verdict 0); 0 otherwise */
  uint32_t tail_added;   /* bases step 1 added to the last exon */
} pgpu_tail_result;      /* 16 bytes */

/* The five steps, in the program's order.  `orig` and `est` are the two sequences of the query, el = est_len; G is the
 * resident sequence, gl its length; every comparison of bytes is plain equality (N is no wildcard, case matters) unless a
 * step says otherwise; "a or A" is the test of the reference's loops.
 *  - Step 1, correct_composition_tail, on orig: with `tail` the last exon, i = tail.EST_end + 1 and j = tail.GEN_end + 1
 *    advance together while i < el, j < gl and orig[i] == G[j]; then tail.EST_end = i - 1, tail.GEN_end = j - 1 and
 *    tail_added is the number of steps.  It runs before the validity test, on whatever the last exon holds.
 *  - Step 2, detect_polyA_signal, on orig and the tail as step 1 left it, the loops as written: with cl = orig + tail.EST_end
 *    + 1 of cll = el - tail.EST_end - 1 bytes, i = matches = 0; while i < cll and not stop: on a or A, stop when matches >= 8,
 *    else count it and go on; on anything else, stop when matches >= 8, else i = cll.  So `stop` needs eight leading a / A
 *    and a ninth byte of any kind.  Only with stop: (a) polyadenil: for i in [max(0, GEN_end - 39), GEN_end], where G[i] is a
 *    or A, the six bytes from i -- fewer where the sequence ends, and then no match -- equal aataaa, AATAAA, attaaa or ATTAAA.
 *    (b) i = max(0, GEN_end - 9), matches = 0; while i <= GEN_end + 10, stop and i < gl: if matches >= 6, stop = false;
 *    otherwise a or A counts and anything else sets matches to 0, and i advances.  (c) with stop still: i = GEN_end + 1, count
 *    = 0; while i <= GEN_end + 10, stop and i < gl: if count >= 7, stop = false; otherwise a or A counts, and i advances.  Each
 *    of (b) and (c) tests its counter before it reads: a counter that fills on the last byte the loop may read cancels
 *    nothing.  polyA = stop.  Both flags are reported whatever step 3 says.
 *  - Step 3, remove_invalid_factorizations: verdict 1 when some exon has EST_start > EST_end or GEN_start > GEN_end, or some
 *    adjacent pair has exon[i].EST_end >= exon[i + 1].EST_start or exon[i].GEN_end >= exon[i + 1].GEN_start.  On verdict 1
 *    out_exons is what step 1 left, the steps are 0, n_kept and recovered are 0; tail_added and the flags stay.
 *  - Step 4, recover_lost_prefixes_and_suffixes, on est.  Both windows are taken from the exons as step 1 left them, then
 *    both answers are applied.  Prefix, with f the first exon, only when f.EST_start > 0 and f.GEN_start > 0: flen = min(
 *    f.EST_start, f.GEN_start), cap = (int)((1.0 + 0.17) * flen) in double arithmetic, elen = min(f.EST_start, cap), glen =
 *    min(f.GEN_start, cap); the windows are read BACKWARDS from the exon: e[i] = est[f.EST_start - 1 - i], g[i] = G[f.GEN_start
 *    - 1 - i].  When e[0] == g[0] nothing is asked.  Otherwise find_longest_affix(e, elen, g, glen) -- PGPU_DP_AFFIX's answer,
 *    bit for bit, a tie in weight going to the cell scanned later -- and when it is valid f.EST_start -= its EST cut,
 *    f.GEN_start -= its genomic cut.  Suffix, with l the last exon, only when el - l.EST_end > 1 and gl - l.GEN_end > 1: flen =
 *    min(el - l.EST_end - 1, gl - l.GEN_end - 1) and both windows have flen bytes (the reference's `(int)(1.0 + rate) * flen`
 *    is 1 * flen), starting ON the exon's last byte: est + l.EST_end, G + l.GEN_end.  Equal first bytes: nothing is asked.
 *    Otherwise the same DP, forwards, and when valid l.EST_end += its EST cut, l.GEN_end += its genomic cut.
 *  - Step 5, remove_false_small_exons / analyze_possibly_small_exon, on est: the exons are walked with prev / curr / next.  An
 *    exon without a prev or a next, or of more than PGPU_TAIL_UB_MED_EXON EST bytes, is not analysed.  Otherwise, with A =
 *    PGPU_TAIL_AFFIXES_LENGTH: estart = max(prev.EST_start + 1, prev.EST_end + 1 - A), eend = min(next.EST_end, next.EST_start
 *    + A), epreflen = prev.EST_end + 1 - estart, esufflen = eend - next.EST_start, allelen = eend - estart, and gstart, gend,
 *    gpreflen, gsufflen, allglen the same on G.  Three edit distances (compute_edit_distance: PGPU_DP_ED's answer, and 0
 *    without a DP when the two strings are equal): the exon against its genomic bytes; est[estart, +epreflen) against
 *    G[gstart, +gpreflen); and the "suffix" pair the reference takes IN FRONT of the window start, est[estart - esufflen,
 *    +esufflen) against G[gstart - gsufflen, +gsufflen), which is 0 unless estart >= esufflen and gstart >= gsufflen (the
 *    reference reads in front of its strings there).  Then general_refine_borders(est + estart, allelen, G + gstart, allglen)
 *    with p0 = 0, p1 = allelen, max_errs = the three distances summed and tail = min(2, gl - gend): PGPU_DP_BORDERS's answer.
 *    The genomic window spans two introns and has no cap: only its first and last min(allelen + max_errs, allglen) bytes are
 *    read.  Refused (ok == 0): outcome 1.  Otherwise new = getBursetFrequency_adaptor(G, gstart + off_t1, gstart + off_t2)
 *    and old = the adaptor's values at (prev.GEN_end + 1, curr.GEN_start) and at (curr.GEN_end + 1, next.GEN_start), summed;
 *    2 * new < old: outcome 2, nothing changes.  Else (equality included) outcome 3: prev.EST_end = estart + off_p - 1,
 *    next.EST_start = eend + off_p - allelen, prev.GEN_end = gstart + off_t1 - 1, next.GEN_start = gend + off_t2 - allglen,
 *    curr is removed, and the merged prev is analysed again as curr, with the exon before it as prev (none at the head) and
 *    the same next.  After any other outcome the walk moves on by one exon.  The reference asserts off_t1 <= off_t2; here a
 *    merge with off_t1 > off_t2 is made as the host code makes it, and a later analysis that finds prev.GEN_end >=
 *    curr.GEN_start or curr.GEN_end >= next.GEN_start (where the reference's unsigned lengths would wrap) is outcome 1.
 *  - out_exons (n_exons_total entries) and out_steps (n_exons_total bytes) are parallel to exons; exons no query names are
 *    copied, with step 0.  out_steps[i]: bits 0-1 the outcome of the last analysis of that exon in step 5 (0 not analysed,
 *    1 refinement refused, 2 accepted but the Burset frequency fell, 3 removed); bit 4: a prefix was recovered into this
 *    exon; bit 5: a suffix; bit 6: step 1 moved its end.  A removed exon's out_exons entry holds it as it was when removed.
 *    n_kept = n_exons less the removed ones.
 *  - Caps refuse only the query that meets them, and only when the DP they bound would run: more than PGPU_TAIL_MAX_EXONS
 *    exons; an affix window of more than PGPU_TAIL_MAX_AFFIX EST bytes whose first bytes differ; an analysis whose allelen
 *    exceeds PGPU_TAIL_MAX_SMALL_WINDOW; an analysed exon of more than PGPU_TAIL_MAX_SMALL_GEN genomic bytes (its strings
 *    cannot be equal, so its edit distance would run).  The result is PGPU_ERANGE with every other field 0, the exons are
 *    copied as they came in and their steps are 0, whichever step met the cap.
 *  - PGPU_EINVAL for the whole call: what pgpu_index_gap_chains lists for the fields the two query structs share (with
 *    est_len == 0), orig_off + est_len > ests_len, and any exon coordinate outside [0, est_len) on the EST or [0, gl) on the
 *    sequence.  Order between the exons is no rule of the input: it is step 3's verdict.
 *  - n == 0 is PGPU_OK (out_exons = exons, out_steps = 0).  idx may be built or loaded. */
int pgpu_index_tail_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                           const pgpu_factor* exons, size_t n_exons_total, const pgpu_tail_query* q, size_t n,
                           pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_tail_chains on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_tail_chains_kernel_ms(void);
/* The same entry with one cap lifted: an affix window of up to PGPU_TAIL_WIDE_MAX_AFFIX EST bytes (a prefix's genomic
 * window is then at most (int)(1.17 * 1024) = 1198 bytes).  Signature, validation, layouts, every other cap and every
 * refusal are pgpu_index_tail_chains'.  The answer equals that entry's, byte for byte, wherever that entry answers: the
 * call runs its kernel first, then a second kernel over the same arrays that takes only the queries left at PGPU_ERANGE
 * and answers them from the input again; one that meets another cap stays PGPU_ERANGE.
 * pgpu_index_tail_chains_kernel_ms reports this call too: both kernels, one event pair. */
int pgpu_index_tail_chains_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                const pgpu_factor* exons, size_t n_exons_total, const pgpu_tail_query* q, size_t n,
                                pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out);

/* The last two routines of refine_EST_factorizations (src/factorization-refinement.c:1270-1305) that concern one
 * factorization alone, chained: search_for_new_small_exons (:875-912, with search_small_exon_at_prefix :500-606 and
 * search_small_exon :641-871) and clean_factorizations (:914-950).  One query = one factorization, as
 * pgpu_index_tail_chains leaves it (the exons it removed taken out); the call is synchronous and batched like that entry.
 * pgpu_index_tail_chains followed by this entry is the whole of refine_EST_factorizations for an EST with one
 * factorization.  add_if_not_exists compares factorizations with each other and stays with the caller.  Nothing in the
 * library calls this entry yet. */
#define PGPU_SMALL_MAX_EXONS          64   /* exons of a query on entry; the list can grow to 2 * n_exons */
#define PGPU_SMALL_MAX_PREFIX_WINDOW 256   /* rows (EST bytes, allelen) of the prefix search's BORDERS: lev_wave_body<4,
                                              BORDERS>, four rows per lane; small_kernel has no scratch and no spilled
                                              vector register with it */
#define PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW 1024   /* the same rows in pgpu_index_small_chains_wide: sixteen per lane */
#define PGPU_SMALL_MAX_KBAND          31   /* as step 5 of pgpu_index_clean_chains: a genomic exon length above 1 033 */
typedef pgpu_tail_query pgpu_small_query;      /* est_off = the WORKING sequence (steps 1-2), orig_off = the ORIGINAL (step 3) */
typedef struct { int32_t min_intron_length; uint32_t reserved; } pgpu_small_params;   /* 8 bytes; config->min_intron_length, any value */
typedef struct {
  int32_t  status;        /* PGPU_OK or PGPU_ERANGE */
  uint8_t  refused;       /* with PGPU_ERANGE, which rule: 1 exons, 2 prefix window, 3 prefix common factor not answerable
                             from the suffix array, 4 K-band bound, 5 exons not in order; 0 with PGPU_OK */
  uint8_t  verdict;       /* 0 kept; 1 emptied by clean_noisy_exons, 2 by clean_external_exons */
  uint8_t  prefix_added;  /* 1: search_small_exon_at_prefix inserted an exon */
  uint8_t  reserved;
  uint32_t n_added;       /* exons inserted by steps 1 and 2 together */
  uint32_t n_list;        /* exons of the list after step 2, written at out_exons[2 * first_exon ..) */
  uint32_t first_kept, n_kept;   /* the run step 3 keeps, relative to that list; 0, 0 unless verdict 0 */
} pgpu_small_result;      /* 24 bytes, no padding */

/* The three steps.  `est` and `orig` are the two sequences of the query; G is the resident sequence, gl its length; MIL is
 * params->min_intron_length.  The list grows, so out_exons and out_steps have 2 * n_exons_total entries: a query writes its
 * list at 2 * first_exon (queries share no exon, so the lists do not meet), and every slot no query fills is written as 0.
 *  - Step 1, search_small_exon_at_prefix (:500-606), on est, only when the first exon p1 has EST_start > 6.  With e1len,
 *    g1len the exon's two lengths: nothing happens unless e1len + p1.EST_start >= 6 + 23 (:517).  eplen = min(p1.EST_start,
 *    p1.GEN_start, 46), epfact = est + p1.EST_start - eplen.  (cflen, pg, pe) = find_longest_common_factor_dp(G[0 ..
 *    p1.GEN_start), epfact): PGPU_DP_LCF's answer -- longest, then smallest start in G, then in the EST piece, N a wildcard.
 *    cflen < 6: nothing happens.  edp = the edit distance of the exon's first min(e1len, g1len, 23) bytes on est and on G
 *    (PGPU_DP_ED's answer; 0 without a DP when the strings are equal), computed only when cflen >= 6.  `pe` is an offset
 *    inside epfact, and the reference uses it as an absolute EST coordinate from here on (:549-603); so does this entry:
 *    allelen = min(p1.EST_end + 1, p1.EST_start + 23) - pe, allglen = min(p1.GEN_end + 1, p1.GEN_start + 23) - pg, both
 *    long when EST_start > 46.  allelen < 12: nothing happens (the host code's return: general_refine_borders has no cut
 *    to try).  Otherwise general_refine_borders(est + pe, allelen, G + pg, allglen) with p0 = 6, p1 = allelen - 6, max_errs =
 *    edp and tail = min(2, gl - (pg + allglen)): PGPU_DP_BORDERS's answer; only the first and last min(allelen + edp,
 *    allglen) genomic bytes are read.  Then the four tests of :568-583 in order: the refinement is ok; (int)off_t2 -
 *    (int)off_t1 >= MIL (the raw value, as int); G[pg + off_t1 ..] begins GT and G[.. pg + off_t2 - 1] ends AG, or gt and ag
 *    (is_canonical_intron :481-494: no mixed case, no GC; with MIL <= 0 the two pairs can lie in front of G, where the
 *    reference reads outside its string: here a byte outside G is no match); off_p - pe >= 6 in unsigned arithmetic (so
 *    off_p < pe passes).
 *    The new exon (pe, pe + off_p - 1, pg, pg + off_t1 - 1) goes in front of p1, and p1.EST_start = pe + off_p,
 *    p1.GEN_start = pg + off_t2.
 *  - Step 2, search_small_exon (:641-871), on est, for every adjacent pair (p1, p2) left to right; after an insertion the
 *    walk goes on with (the old p2, its successor): the new exon is never analysed.  Nothing happens unless e1len + e2len
 *    >= 6 + 2 * 23 (:664).  e1slen = min(e1len, g1len, 23): the last e1slen bytes of p1 on est and on G; e2plen = min(e2len,
 *    g2len, 23): the first e2plen bytes of p2 on both.  sed and ped are the two edit distances (0 for equal strings, else
 *    PGPU_DP_ED).  The search goes on only when sed + ped > 2 or classify(p1.GEN_end + 1, p2.GEN_start - 1) == 2
 *    (pgpu_index_classify's answer).  A side whose distance is > 0 asks find_longest_common_factor_dp of its two strings
 *    (EST piece first; PGPU_DP_LCF's answer) for (f1slen, e1socc, g1socc) or (f2plen, e2pocc, g2pocc); a side with distance
 *    0 has its whole length and 0, 0.  The extension loop of :725-737 as written.  elen = (e1slen - e1socc) + (e2pocc +
 *    f2plen) - 12, estart = p1.EST_end + 1 - e1slen + e1socc + 6, allgstart = p1.GEN_end + 1 - e1slen + g1socc + 6, allglen =
 *    p2.GEN_start + g2pocc + f2plen - 6 - allgstart.  Then exactly one pgpu_sexon_query: (est + estart, elen, allgstart,
 *    allglen, f1slen, f2plen, max(4, MIL) as int) through the search of pgpu_index_small_exons, which holds the four gates
 *    of :743-758; the window ends inside p2, so it cannot pass the end of G; an elen below 0 finds nothing (an exon shorter than a
 *    border whose match the loop of :725-737 lengthened: the reference's unsigned elen wraps and its copy leaves the EST).  A result of length >= 6 is accepted with the four cut
 *    assignments of :836-866: the new exon (estart + offstart, .. + len - 1, gpos, gpos + len - 1) goes between p1 and p2,
 *    p1.EST_end = estart + offstart - 1, p1.GEN_end = allgstart + offstart - 1, p2.EST_start = estart + offstart + len,
 *    p2.GEN_start = allgstart + allglen - offend.
 *  - Step 3, clean_factorizations (:914-950), on orig: step 5 of pgpu_index_clean_chains over the whole list
 *    (clean_noisy_exons with only_internals = false: per exon K_band_edit_distance with the bound of its genomic length, an
 *    exon with GEN_start > GEN_end counted as noisy, then the best-run rule), verdict 1 when nothing is left; then step 3
 *    of pgpu_index_clean_chains on the run that is left (clean_external_exons: byte comparison for "distance > 0"), verdict
 *    2 when nothing is left.  In this order, which is not that entry's.
 *  - out_steps, per exon of the list: bit 0 inserted by step 1; bit 1 inserted by step 2; bit 2 an end of this exon was
 *    moved by an insertion beside it; bit 4 the K-band verdict of step 3 was false; bit 5 dropped by clean_external_exons.
 *  - Refusals are per query: PGPU_ERANGE and `refused`, every other field 0, the query's exons copied unchanged to
 *    out_exons[2 * first_exon ..) with steps 0.  A cap refuses only when the computation it bounds would run.  1: more than
 *    PGPU_SMALL_MAX_EXONS exons.  2: step 1 reaches its border refinement with allelen > PGPU_SMALL_MAX_PREFIX_WINDOW.  3:
 *    step 1 reaches its common factor and the suffix array cannot answer it: p1.GEN_start beyond the first byte of G that
 *    is no upper-case A, C, G or T (an exon that begins ON that byte is answered: the intron step 1 tests may lie at or
 *    behind p1.GEN_start, lower case included), or a byte of epfact that is none of those, other than a single N or n.  4: step 3 meets
 *    an exon with GEN_start <= GEN_end whose bound exceeds PGPU_SMALL_MAX_KBAND.  5: an exon with start > end, or two
 *    adjacent exons that are not strictly increasing (p1 end < p2 start) on either string -- the reference asserts this
 *    (:512-513, :655-658), and step 5 of pgpu_index_tail_chains can hand over such a list.
 *  - PGPU_EINVAL for the whole call: what pgpu_index_tail_chains lists, with its coordinate rule, and params == NULL or
 *    params->reserved != 0.
 *  - n == 0 is PGPU_OK (out_exons and out_steps all 0).  idx may be built or loaded; the classification tables are built
 *    on first use as for pgpu_index_small_exons. */
int pgpu_index_small_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                            const pgpu_factor* exons, size_t n_exons_total, const pgpu_small_query* q, size_t n,
                            const pgpu_small_params* params,
                            pgpu_factor* out_exons /* 2 * n_exons_total */, uint8_t* out_steps /* 2 * n_exons_total */,
                            pgpu_small_result* out);
/* HIP-event time of the kernel of the calling thread's last pgpu_index_small_chains on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_small_chains_kernel_ms(void);
/* The same entry with one cap lifted: step 1's border refinement takes an allelen of up to
 * PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW.  Signature, validation, layouts, every other cap and every refusal are
 * pgpu_index_small_chains'.  The answer equals that entry's, byte for byte, wherever that entry answers: the call runs
 * its kernel first, then a second kernel over the same arrays that takes only the queries with refused == 2 and answers
 * them from the input again; one that then meets another cap is refused with that cap's code, and an allelen beyond the
 * wide cap stays refused == 2.  pgpu_index_small_chains_kernel_ms reports this call too: both kernels, one event pair. */
int pgpu_index_small_chains_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                 const pgpu_factor* exons, size_t n_exons_total, const pgpu_small_query* q, size_t n,
                                 const pgpu_small_params* params,
                                 pgpu_factor* out_exons /* 2 * n_exons_total */, uint8_t* out_steps /* 2 * n_exons_total */,
                                 pgpu_small_result* out);

/* ------------------------------------------------------------------------------------------ */
/* pairings -- replaces build_vertex_set (src/max-emb-graph.c:218-392): for every position p   */
/* of every pattern, the maximal pairings (p, t, l) of the pattern with the genomic, after the  */
/* two low-complexity filters, in the order of the reference's per-position lists.            */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t min_factor_len;         /* config->min_factor_len (+ inc_pairing_len)  */
  uint32_t reserved;
  double   min_string_depth_rate;  /* config->min_string_depth_rate               */
} pgpu_pairing_params;

typedef struct { int32_t p, t, l; } pgpu_pairing;

/* patterns: concatenated pattern bytes; pat_off[i]..pat_off[i+1] delimits pattern i (n_pat+1
 * offsets).  out/out_cap: caller buffer for pairings; out_first[i]..out_first[i+1] delimits the
 * pairings of pattern i (n_pat+1 entries), sorted by (p, t, l) as pairing_compare orders them
 * (src/types.c:391-411).  Returns PGPU_ENOSPC (and the needed count in *n_out) when out_cap is
 * too small. */
int pgpu_pairings(pgpu_ctx* ctx, const pgpu_index* idx,
                  const char* patterns, const uint64_t* pat_off, size_t n_pat,
                  const pgpu_pairing_params* params,
                  pgpu_pairing* out, size_t out_cap, uint64_t* out_first, size_t* n_out);

/* The same in three steps for callers that keep the patterns resident (bench, batched host):
 * create uploads the patterns; run launches every kernel with the given parameters (may be
 * repeated with other parameters: the reference re-runs build_vertex_set with a longer
 * min_factor_len when a MEG is too complex, src/compute-est-fact.c:132-144); fetch downloads.
 * The stages of a plan build on each other -- run, run_meg, run_candidates, run_factorizations,
 * run_final_factorizations, below -- and the run
 * of a stage takes with it what the stages behind it had made.  On a plan with patterns a fetch whose stage's results
 * are not there (never made, or gone with a later run of an earlier stage) is PGPU_EINVAL with a message, never
 * stale data. */
typedef struct pgpu_pairing_plan pgpu_pairing_plan;
int pgpu_pairing_plan_create(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                             const uint64_t* pat_off, size_t n_pat, pgpu_pairing_plan** plan);
/* The same plan (build_vertex_set, src/max-emb-graph.c:218-392, as above) for a batch that is cut into several
 * plans used one after the other (the chunks of the EST batch the host prefetches): only the patterns -- bytes, offsets, 2-bit packing -- are the plan's own, in ONE
 * device allocation; every buffer a run writes (16 of them, ~60 bytes per pattern position, and the MEG stage's
 * 11 KB per pattern) is shared by all resident plans of the context.  What a run leaves -- the pairings for
 * fetch / run_meg, the MEG records for fetch_meg -- is valid until another resident plan of the same context
 * runs; asking later is PGPU_EINVAL, never stale data.  (A one-shot process made 200 allocations of 7 GB for
 * its ten chunks before this: a third of its first step.) */
int pgpu_pairing_plan_create_resident(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns,
                                      const uint64_t* pat_off, size_t n_pat, pgpu_pairing_plan** plan);
int pgpu_pairing_plan_run(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_pairing_params* params);
uint64_t pgpu_pairing_plan_count(const pgpu_pairing_plan* plan);       /* pairings of the last run */
uint64_t pgpu_pairing_plan_positions(const pgpu_pairing_plan* plan);   /* pattern positions */
/* HIP-event time of stage k of the last run: 0 locate, 1 chain, 2 count+scan, 3 fill,
 * 4 cross+scan, 5 emit */
double pgpu_pairing_plan_kernel_ms(const pgpu_pairing_plan* plan, int k);
int pgpu_pairing_plan_fetch(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_pairing* out, size_t out_cap,
                            uint64_t* out_first);
int pgpu_pairing_plan_destroy(pgpu_ctx* ctx, pgpu_pairing_plan* plan);

/* ------------------------------------------------------------------------------------------ */
/* maximal-embedding graphs -- for every pattern of a plan whose pairings have just been       */
/* computed (pgpu_pairing_plan_run), the rest of build_meg (src/compute-est-fact.c:101-131):    */
/* build_edge_set (src/max-emb-graph.c:650-676 with is_there_an_edge_strict :394-465,           */
/* add_edges_from :533-553, add_edges_from_source :555-599, add_edges_to_sink :601-647),        */
/* simplify_meg (src/meg-simplification.c:314,193-232,142-191), transitive_reduction            */
/* (:333-632), compact_short_edges (:258-312), is_too_complex_for_compaction and                */
/* is_too_complex (:68-139).  The pairings stay in HBM; what comes back is the finished graph.  */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t min_factor_len;            /* the one the pairings were computed with            */
  int32_t  min_intron_length, max_intron_length;
  uint32_t max_pairings_in_MEG;
  double   max_prefix_discarded_rate, max_suffix_discarded_rate, max_freq_shortest_pairing;
  uint32_t trans_red, short_edge_comp;   /* booleans                                         */
} pgpu_meg_params;

#define PGPU_MEG_MAX_VERTICES 64      /* vertices ever created for one MEG (source and sink included) */
#define PGPU_MEG_MAX_DEGREE   32      /* out- or in-degree of a vertex                                 */
#define PGPU_MEG_TOO_COMPLEX  1u      /* too_complex of build_meg (:122-131): the caller retries        */
#define PGPU_MEG_UNAVAILABLE  2u      /* beyond the limits above (or cyclic): the record is a bare
                                         header and the caller builds this MEG from the pairings       */
/* One record per pattern, 4-byte aligned, little endian:
 *   u32 n_vertices, u32 n_edges, u32 flags, u32 0
 *   n_vertices x (i32 p, t, l)     in the order of the reference's position lists = the numbering
 *                                  meg_write prints (src/io-meg.c:161-170); [0] source, [last] sink
 *   (n_vertices + 1) x u16         first edge of each vertex (CSR)
 *   n_edges x u8                   target vertex, in the order of the reference's adjacency lists
 *   (pad to 4) u32 meg_text_len, u32 edges_text_len, then the two texts est-fact prints for this
 *                                  graph: meg_write's "(p,t,l)" lines, "#adj#", "i-j" lines
 *                                  (src/io-meg.c:146-190) and the lines of
 *                                  add_intronic_edges_to_file (src/max-emb-graph.c:677-699)
 * run_meg builds the records of all patterns (after pgpu_pairing_plan_run with the same
 * min_factor_len); meg_bytes = total size; fetch_meg copies them and the n_pat + 1 byte offsets. */
int pgpu_pairing_plan_run_meg(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_meg_params* params);
uint64_t pgpu_pairing_plan_meg_bytes(const pgpu_pairing_plan* plan);
int pgpu_pairing_plan_fetch_meg(pgpu_ctx* ctx, pgpu_pairing_plan* plan, void* out, size_t out_cap,
                                uint64_t* rec_first);
/* HIP-event time of the MEG kernels of the last run_meg (build + scan + emit) */
double pgpu_pairing_plan_meg_ms(const pgpu_pairing_plan* plan);

/* ------------------------------------------------------------------------------------------ */
/* candidates -- the factorization of a MEG that is one path, from its record: what            */
/* get_EST_factorizations does between the graph and the cleaning steps of                      */
/* pgpu_index_clean_chains when get_subtree_embeddings (src/est-factorizations.c:597-762) has   */
/* one embedding per vertex: update_embedding (:765-917, the Burset cut scan included) folded   */
/* over the path from the sink backwards, then get_factorizations_from_embeddings               */
/* (:1292-1356).  One record = one candidate at most; its exons have the shape the chained      */
/* entries above take (run -> run_meg -> run_candidates -> clean -> gaps -> refine).            */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t min_factor_len;     /* config->min_factor_len as the MEG was built with; 1 .. 2^24 */
  int32_t  min_intron_length;  /* config->min_intron_length; only compared: any value         */
} pgpu_cand_params;          /* 8 bytes */

#define PGPU_CAND_NONE     0u   /* the record is flagged (PGPU_MEG_UNAVAILABLE or PGPU_MEG_TOO_COMPLEX): no graph to walk,
                                   or the caller retries with longer factors */
#define PGPU_CAND_NOT_PATH 1u   /* the graph is not one path: the caller enumerates (get_subtree_embeddings) */
#define PGPU_CAND_REFUSED  2u   /* one path, and update_embedding returned NULL for some vertex: no candidate at all */
#define PGPU_CAND_ONE      3u   /* one path, one embedding, one candidate */
typedef struct {
  uint32_t kind;               /* PGPU_CAND_* */
  uint32_t work;               /* the units the enumeration counts (:626-629, :706-711): n_vertices, plus one per
                                  update_embedding that returned an embedding, up to the refusal when there is one;
                                  0 for NONE and NOT_PATH.  Comparing it with a budget stays with the caller */
  uint32_t first_exon;         /* the candidate = exons[first_exon .. first_exon + n_exons); ONE only */
  uint16_t n_exons;            /* >= 1 for ONE, else 0 */
  uint16_t n_pairs;            /* pairings of the embedding; ONE only */
} pgpu_cand_result;          /* 16 bytes */

/*  - The path test: 2 <= n_vertices <= 64; vertex 0 is the source (p == INT32_MIN); from it the only out-edge is
 *    followed until a vertex without one; no vertex is met twice and none on the way has an out-degree other than 1;
 *    every vertex was visited and the last one is the sink (p == INT32_MAX - 200).  Anything else is NOT_PATH.
 *  - The fold, from the sink backwards, with `head` the first pairing of the embedding so far, `node` the vertex in
 *    front of it, L = min_factor_len and all of it in the reference's int arithmetic (:765-917):
 *      head is the sink: a node with p < 0 (the source) refuses, any other node becomes the embedding;
 *      node is the source: the embedding is copied;
 *      small_delta = head.p + head.l - node.p, big_delta = head.t + head.l - node.t; refused unless both >= 2L,
 *      small_delta - (node.l + head.l) <= 2L and small_delta - big_delta <= 2L;
 *      when both deltas are >= node.l + head.l the two keep their lengths; otherwise the overlap is split:
 *      ref_delta = min(small_delta, big_delta), node gets ref_delta / 2 and head the rest, clamped first on node.l,
 *      else on head.l, and head begins that much in front of its old end on both strings;
 *      gap_on_p / gap_on_t = head's start - node's start - node's length - 1 on either string, intron_len = gap_on_t -
 *      max(gap_on_p, 0), intron_on_t = intron_len >= 0 && (min_intron_length == 0 || intron_len >= min_intron_length);
 *      when small_delta < node.l + head.l and intron_on_t, the cut scan: for cut in [max(node.p + L, head.p),
 *      min(head.p + head.l - L, node.p + node.l)] ascending, f = getBursetFrequency_adaptor(sequence,
 *      cut - node.p + node.t, cut - head.p + head.t), kept when f >= the best so far (which starts at -1): the LAST of
 *      equal cuts wins, and an empty range leaves best_cut = 0 and the arithmetic goes on with it; head then begins at
 *      the cut and node ends in front of it;
 *      refused unless gap_on_t <= 2L || intron_on_t (gap_on_t as it was BEFORE the cut scan).
 *    The adaptor reads the resident sequence as a C string: a byte at or behind its end is the terminator, i.e.
 *    frequency 0; cut2 < 2 gives 0; the lookup is case-insensitive, anything but ACGT gives 0.
 *  - The exons (:1292-1356), over the embedding front to back: a pairing x opens an exon when x.t - GEN_end of the
 *    exon before - 1 > 2L, otherwise it moves that exon's EST_end and GEN_end to its own end.  The embedding is never
 *    stored: a step of the fold fixes the length of the node it adds and the start of the head it trims, nothing older
 *    changes again, so the exons are produced back to front.
 *  - exons of a call are compact, in record order; NONE, NOT_PATH and REFUSED records have none. */

/* Plan form: the candidates of the records pgpu_pairing_plan_run_meg left in HBM; nothing of a record crosses the bus.
 * PGPU_EINVAL (with a message): no run_meg since the last run; min_factor_len 0, above 2^24 or not the MEG stage's; the
 * results of a resident plan were overwritten by the run of another one; fetch before run_candidates.  An empty plan is
 * PGPU_OK.  A rerun gives the same bytes.  The buffers come from where the MEG stage's do. */
int pgpu_pairing_plan_run_candidates(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_cand_params* params);
uint64_t pgpu_pairing_plan_candidate_exons(const pgpu_pairing_plan* plan);   /* exons of the last run_candidates */
/* out: n_pat results; exons: at least candidate_exons entries (PGPU_ENOSPC when exons_cap is smaller) */
int pgpu_pairing_plan_fetch_candidates(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_cand_result* out,
                                       pgpu_factor* exons, size_t exons_cap);
/* HIP-event time of the last run_candidates (count + scan + write); 0 without timing */
double pgpu_pairing_plan_candidates_ms(const pgpu_pairing_plan* plan);

/* Index form: the same for a caller that holds records (fetched ones: a resident plan's results expire with the next
 * chunk's run; or hand-made ones).  records: records_len bytes; rec_first[i] .. rec_first[i + 1] delimits record i
 * (n + 1 offsets); out: n results; *n_exons: exons written.  Synchronous and batched like the other pgpu_index_*
 * queries.
 *  - PGPU_EINVAL for the whole call: a null pointer (no message); min_factor_len 0 or above 2^24; rec_first not
 *    ascending or beyond records_len; a record that is not at a multiple of 4, or shorter than 16 bytes; and in a record
 *    without either flag: one shorter than its header's counts need (16 + 12 n_vertices + 2 (n_vertices + 1) + n_edges);
 *    n_vertices > 64; CSR offsets that are not ascending or go beyond n_edges; a target >= n_vertices; a source or sink
 *    (by its p) whose t is not its p or whose l is not 200; any other vertex, a pairing, with p < 0, l < 0 or
 *    p + l > 2^29, or whose t or t + l lies outside the sequence.  A flagged record is a bare header: nothing behind its
 *    16 bytes is read.
 *  - PGPU_ENOSPC, with the needed count in *n_exons and nothing written to out or exons, when exons_cap is too small.
 *  - n == 0 is PGPU_OK (*n_exons = 0).  idx may be built or loaded. */
int pgpu_index_candidates(pgpu_ctx* ctx, const pgpu_index* idx, const void* records, size_t records_len,
                          const uint64_t* rec_first, size_t n, const pgpu_cand_params* params,
                          pgpu_cand_result* out, pgpu_factor* exons, size_t exons_cap, size_t* n_exons);
/* HIP-event time of the kernels of the calling thread's last pgpu_index_candidates on a context with timing on
 * (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_candidates_kernel_ms(void);

/* ------------------------------------------------------------------------------------------ */
/* candidate lists -- every candidate factorization of a MEG that need not be one path, from   */
/* its record: the enumeration of get_EST_factorizations (src/est-factorizations.c:160-200)    */
/* with get_subtree_embeddings (:597-762: roots in position order, embeddings memoised per     */
/* vertex, the maximality pruning with maximality_relation :1362-1460) and                      */
/* get_factorizations_from_embeddings (:1292-1356).  One record = a list of candidates; each    */
/* candidate is an exon array of the shape the chained entries above take, one query per        */
/* candidate.  What compares candidates with each other (add_if_not_exists, FILTER 1, FILTER 3) */
/* stays with the caller.  The parameters are pgpu_cand_params.                                 */
/* ------------------------------------------------------------------------------------------ */
#define PGPU_ENUM_MAX_LIST        64u   /* entries a vertex's list of embeddings may hold at any moment */
#define PGPU_ENUM_MAX_EMBEDDINGS 512u   /* embeddings that may be created for one record                 */

#define PGPU_ENUM_NONE   0u   /* the record is flagged (PGPU_MEG_UNAVAILABLE or PGPU_MEG_TOO_COMPLEX): as PGPU_CAND_NONE */
#define PGPU_ENUM_CYCLIC 1u   /* the walk met a vertex that is on its own stack (the MEG stage never emits such a graph;
                                 the host's recursion does not end on one) */
#define PGPU_ENUM_RANGE  2u   /* beyond one of the two caps: detail says which; the caller enumerates on the host */
#define PGPU_ENUM_LISTS  3u   /* answered: n_candidates candidates (a record may have none) */
#define PGPU_ENUM_CAP_LIST       1u   /* detail of RANGE: a list held more than PGPU_ENUM_MAX_LIST entries      */
#define PGPU_ENUM_CAP_EMBEDDINGS 2u   /* detail of RANGE: more than PGPU_ENUM_MAX_EMBEDDINGS embeddings created */
typedef struct {
  uint16_t kind;               /* PGPU_ENUM_* */
  uint16_t detail;             /* RANGE: PGPU_ENUM_CAP_*; else 0 */
  uint32_t work;               /* LISTS: one unit per vertex entered plus one per update_embedding that returned an
                                  embedding (:626-629, :706-711); it does not depend on the order of the walk, and on a
                                  record that is one path it is pgpu_cand_result.work.  0 for NONE, CYCLIC and RANGE.
                                  Comparing it with a budget stays with the caller */
  uint32_t first_candidate;    /* the record's candidates = cands[first_candidate .. first_candidate + n_candidates);
                                  LISTS with candidates only, else 0 */
  uint16_t n_candidates;       /* LISTS only (0 .. 512), else 0 */
  uint16_t n_roots;            /* LISTS only: the roots the walk began at, with or without candidates */
} pgpu_enum_result;          /* 16 bytes */
typedef struct {
  uint32_t first_exon;         /* the candidate = exons[first_exon .. first_exon + n_exons) */
  uint16_t n_exons;            /* >= 1 */
  uint16_t n_pairs;            /* pairings of the embedding */
  uint32_t root;               /* index of the root's vertex in the record */
  uint32_t reserved;           /* 0 */
} pgpu_enum_candidate;       /* 16 bytes */

/* Per record, with L = min_factor_len:
 *  - A flagged record is NONE; nothing behind its 16 bytes is read.
 *  - Roots.  The vertices are taken in record order (the reference's position-list order); one that has not been visited
 *    yet is a root.  Entering a vertex's subtree marks it visited, whether or not its embeddings are memoised already.
 *  - embeddings(v), computed once per vertex.  A vertex without out-edges -- any such vertex, not only the sink -- has the
 *    single embedding [v].  Otherwise the adjacent vertices are taken in CSR order, and for every embedding e of
 *    embeddings(adj), in list order, add = update_embedding(e, v): exactly the fold step of the candidate stage above (the
 *    sink and source cases, the split with its two clamps, the Burset cut scan where the last of equal cuts wins).  A NULL
 *    is skipped.  Otherwise add is compared with the list built so far, from its front: k0 is the first entry whose
 *    maximality_relation(add, entry) is 0; the entries in front of k0 (all entries when there is no k0) whose relation is
 *    2 are removed; add is appended only when there is no k0.
 *  - maximality_relation(add, cmp) (:1362-1460), with "x inside y" = x.p >= y.p, x.p + x.l <= y.p + y.l and the same on t,
 *    over the first min(|add|, |cmp|) pairings of both: |add| > |cmp|: 2 when every cmp[i] is inside add[i], else 1;
 *    |add| < |cmp|: 0 when every add[i] is inside cmp[i], else 1; equal lengths: 0 when every add[i] is inside cmp[i],
 *    else 2 when every cmp[i] is inside add[i], else 1.
 *  - Candidates come root by root in root order, and within a root they are the root's embeddings in list order, each
 *    through the exon rule of the candidate stage (a pairing x opens an exon when x.t - GEN_end - 1 > 2L).  Only roots
 *    yield candidates.  A graph of a source and a sink without an edge has two roots and two candidates of one exon each,
 *    which check_for_not_source_sink_factorization drops later; a record without a vertex has neither.
 *  - The caps.  RANGE with PGPU_ENUM_CAP_LIST when a vertex's list holds more than 64 entries behind an append; with
 *    PGPU_ENUM_CAP_EMBEDDINGS when more than 512 embeddings are created for the record, an embedding being created by a
 *    vertex without out-edges or by an update_embedding that returned one (a copy made for the source included, and
 *    whether or not the pruning then keeps it).  CYCLIC when an adjacent vertex is on the walk's own stack.  The walk is
 *    the host's recursion -- depth first, an adjacent vertex's subtree before its embeddings are folded, one adjacent
 *    vertex after the other -- and the first of the three it meets decides.  Such a record reports its kind, the
 *    detail, and zeros.
 *  - A source without out-edges that another vertex has an edge to (no stage emits one) is a head whose deltas leave
 *    what int holds; as integers small_delta is below 2L, so update_embedding returns NULL for it, and that is the rule.
 *  - Candidates of a call are compact in record order, exons in record order and then candidate order; first_candidate
 *    and first_exon index the call's arrays. */

/* Plan form: the candidate lists of the records pgpu_pairing_plan_run_meg left in HBM.  A branch beside the ladder of stages,
 * not a rung: it asks for the records (run_meg with the same min_factor_len), changes nothing of what the plan's other
 * stages hold, and its results stay valid until the next run or run_meg of the plan, or the run of another resident
 * plan; after that fetch_candidate_lists is PGPU_EINVAL with a message.  run_candidates and the stages above it neither
 * need the lists nor disturb them.  PGPU_EINVAL (with a message) as for run_candidates.  An empty plan is PGPU_OK.  A
 * rerun gives the same bytes. */
int pgpu_pairing_plan_run_candidate_lists(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_cand_params* params);
/* candidates and exons of the last run_candidate_lists (either pointer may be null) */
int pgpu_pairing_plan_candidate_list_counts(const pgpu_pairing_plan* plan, uint64_t* n_cands, uint64_t* n_exons);
/* out: n_pat results; PGPU_ENOSPC when cands_cap or exons_cap is smaller than the counts */
int pgpu_pairing_plan_fetch_candidate_lists(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_enum_result* out,
                                            pgpu_enum_candidate* cands, size_t cands_cap, pgpu_factor* exons, size_t exons_cap);
/* HIP-event time of the last run_candidate_lists (count + two scans + write); 0 without timing */
double pgpu_pairing_plan_candidate_lists_ms(const pgpu_pairing_plan* plan);

/* Index form: records, offsets, parameters and every PGPU_EINVAL as pgpu_index_candidates (the same validator).  out: n
 * results; *n_cands, *n_exons: candidates and exons written.  PGPU_ENOSPC, with both needed counts in *n_cands and
 * *n_exons and nothing written to out, cands or exons, when cands_cap or exons_cap is too small.  n == 0 is PGPU_OK (both
 * counts 0).  PGPU_EINVAL (with a message) when a call's candidates or exons pass 2^32 - 1, which first_candidate and
 * first_exon could not index: only a call of more than 131 071 records can.  idx may be built or loaded. */
int pgpu_index_candidate_lists(pgpu_ctx* ctx, const pgpu_index* idx, const void* records, size_t records_len,
                               const uint64_t* rec_first, size_t n, const pgpu_cand_params* params,
                               pgpu_enum_result* out, pgpu_enum_candidate* cands, size_t cands_cap,
                               pgpu_factor* exons, size_t exons_cap, size_t* n_cands, size_t* n_exons);
/* HIP-event time of the kernels of the calling thread's last pgpu_index_candidate_lists (as
 * pgpu_index_candidates_kernel_ms); 0 without timing */
double pgpu_index_candidate_lists_kernel_ms(void);

/* ------------------------------------------------------------------------------------------ */
/* factorizations -- a candidate taken through the cleaning steps (pgpu_index_clean_chains),   */
/* check_gap_errors (pgpu_index_gap_chains) and the refinement loop (pgpu_index_refine_chains)  */
/* in ONE call, nothing leaving HBM in between: for an EST with exactly one candidate this is   */
/* all that get_EST_factorizations (src/est-factorizations.c) does between the graph and        */
/* correct_tail -- FILTER 1 and FILTER 3 compare a candidate with the best one and are no-ops   */
/* on one (max_cov - c == 0, g - min_gl == 0); max_number_of_factorizations stays with the      */
/* caller.  The three stage kernels are the ones of the chained entries; between them one       */
/* thread per EST does what a caller of those entries does on the host: cut the kept run out of */
/* clean's answer, drop the exons gaps merged, build the next query.                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  double  complexity_threshold;       /* clean: config->complexity_threshold */
  int32_t suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen;   /* refine: each in [0, 2^24] */
  int32_t min_intron_length;          /* refine: config->min_intron_length; only compared: any value */
} pgpu_fact_params;          /* 24 bytes: 0, 8, 12, 16, 20; no padding */

#define PGPU_FACT_HOST  0u   /* no answer from the device: the caller runs its own path from the MEG record */
#define PGPU_FACT_EMPTY 1u   /* the answer is "no factorization" */
#define PGPU_FACT_DONE  2u   /* exons[first_exon .. first_exon + n_exons): the factorization as the loop of
                                est-factorizations.c:446-490 leaves it, the first-exon rule (:476-485) applied */
typedef struct {
  uint8_t  outcome;          /* PGPU_FACT_* */
  uint8_t  stage;            /* where the outcome fell: 0 candidate, 1 clean, 2 gaps, 3 refine */
  uint16_t detail;           /* HOST: at stage 0 the candidate's kind (PGPU_CAND_NONE, PGPU_CAND_NOT_PATH); at stages 1-3:
                                1 a cap (that entry's PGPU_ERANGE for the query), 2 an input that entry's validator refuses
                                (for a whole call, there; for this EST alone, here).
                                EMPTY: at stage 0 PGPU_CAND_REFUSED; at stage 1 clean's verdict 1 .. 7; at stage 2: 1.
                                DONE: bit 0 = dropped_first of pgpu_chain_result (the exon is not among the n_exons) */
  uint32_t first_exon;       /* DONE only, else 0: into the call's compact exon array */
  uint16_t n_exons;          /* DONE only (>= 1), else 0 */
  uint16_t n_merged;         /* DONE only, else 0: exons check_gap_errors merged into the one before them */
  uint32_t total_edit;       /* tot_out_edit_distance of check_gap_errors whenever the gaps stage answered (EMPTY at stage 2,
                                every outcome at stage 3); else 0 */
} pgpu_fact_result;          /* 16 bytes: outcome 0, stage 1, detail 2, first_exon 4, n_exons 8, n_merged 10, total_edit 12 */

/*  - The stages, per EST, each exactly the chained entry of that name on a query of its own:
 *    0. the candidate: none (HOST, detail = the kind), refused by update_embedding (EMPTY), or one list of exons;
 *    1. clean with complexity_threshold.  What pgpu_index_clean_chains refuses for a whole call is HOST with detail 2 for
 *       this EST: an exon coordinate outside [-1, est_len] / [-1, length of the sequence], an empty EST, or, for a list that
 *       passes step 1, an end exon that begins in front of or ends behind its string.  PGPU_ERANGE is HOST with detail 1,
 *       verdict 1 .. 7 is EMPTY (also 7, whose kept run the chained entry reports: there is no factorization);
 *    2. gaps on the kept run [first_kept, first_kept + n_kept) of clean's out_exons.  Two adjacent exons out of order on
 *       either string or an EST gap longer than its genomic gap: HOST, detail 2.  PGPU_ERANGE: HOST, detail 1.  Verdict 1:
 *       EMPTY, detail 1;
 *    3. refine on the exons gaps kept (out_steps without bit 7), donors with their merged ends, with the four settings of
 *       the call.  Two adjacent exons not strictly in order: HOST, detail 2.  PGPU_ERANGE: HOST, detail 1 (the partly
 *       refined chain is not reported).  Otherwise DONE: the chain's out_exons, less the first one when dropped_first.
 *  - exons and steps of a call are compact, in EST order; only DONE has any.  steps[k] is pgpu_index_refine_chains'
 *    out_steps of that exon: path in bits 0-3, refined in bit 7, for the intron in front of it; 0 for the first exon of the
 *    chain (after dropped_first the list begins with the chain's second exon, which keeps its byte).
 *  - An outcome never depends on another EST of the call: an EST with nothing to do at a stage is given that stage's
 *    trivial query (clean: one exon with EST_start = -1; gaps and refine: one exon) on a placeholder exon of its own.
 *  - Comparing pgpu_cand_result.work with a budget stays with the caller, as for the candidate stage. */

/* Plan form: the candidates of the last pgpu_pairing_plan_run_candidates, where they lie; the ESTs are the plan's patterns.
 * ONE goes down the chain, REFUSED is EMPTY at stage 0, NONE and NOT_PATH are HOST at stage 0.  The candidates stay
 * fetchable and unchanged.  PGPU_EINVAL (with a message): no run_candidates since the last run or run_meg; the results of
 * a resident plan were overwritten by the run of another one; a suffpref length outside [0, 2^24]; more than 2^31 - 1
 * patterns or candidate exons (as the index form); fetch before run_factorizations.  An empty plan is PGPU_OK.  A rerun
 * gives the same bytes.  The buffers come from where the MEG stage's do.  One host wait lies inside the call (8 bytes: the
 * workspace the end-exon alignments of clean need). */
int pgpu_pairing_plan_run_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_fact_params* params);
uint64_t pgpu_pairing_plan_factorization_exons(const pgpu_pairing_plan* plan);   /* exons of the last run_factorizations */
/* out: n_pat results; exons, steps: at least factorization_exons entries (PGPU_ENOSPC when cap is smaller) */
int pgpu_pairing_plan_fetch_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_fact_result* out, pgpu_factor* exons,
                                           uint8_t* steps, size_t cap);
/* HIP-event times of the last run_factorizations: k = 0 the whole call (hand-off kernels, the host wait, the scan
 * included), 1 clean_kernel, 2 gaps_kernel, 3 chain_kernel; 0 without timing */
double pgpu_pairing_plan_factorizations_ms(const pgpu_pairing_plan* plan, int k);

/* Index form: the same driver for a caller that holds candidates (fetched ones, or hand-made ones).  One query = one EST:
 * the fields of pgpu_gaps_query, where n_exons == 0 means "no candidate" (HOST at stage 0, detail PGPU_CAND_NONE; first_exon
 * is then not looked at).  out: n results; out_exons, out_steps: cap entries; *n_out: exons written.  One upload, one
 * download; synchronous and batched like the other pgpu_index_* queries.
 *  - PGPU_EINVAL for the whole call only for structure: a null pointer (no message); est_off + est_len > ests_len or
 *    first_exon + n_exons > n_exons_total; est_len == 0 or > 2^31 - 1; reserved != 0; two queries share an exon; a suffpref
 *    length outside [0, 2^24]; more than 2^31 - 1 queries or exons.  Whatever concerns the VALUES of the exons, factor
 *    coordinates outside their strings included, is HOST with detail 2 for that query, exactly as in the plan form.
 *  - PGPU_ENOSPC, with the needed count in *n_out and nothing written to out, out_exons or out_steps, when cap is too small.
 *  - n == 0 is PGPU_OK (*n_out = 0).  idx may be built or loaded. */
typedef pgpu_gaps_query pgpu_fact_query;     /* 24 bytes */
int pgpu_index_factorizations(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_factor* exons,
                              size_t n_exons_total, const pgpu_fact_query* q, size_t n, const pgpu_fact_params* params,
                              pgpu_fact_result* out, pgpu_factor* out_exons, uint8_t* out_steps, size_t cap, size_t* n_out);
/* HIP-event time of the whole device part of the calling thread's last pgpu_index_factorizations on a context with timing
 * on (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_factorizations_kernel_ms(void);

/* ------------------------------------------------------------------------------------------ */
/* factorization lists -- every candidate of one EST (pgpu_index_candidate_lists' output as it  */
/* is) to the list of factorizations get_EST_factorizations (src/est-factorizations.c:203-490)  */
/* holds just before correct_composition_tail: the cleaning steps per candidate,               */
/* add_if_not_exists (:2041-2109) folded over the survivors, FILTER 1 (:278-331), FILTER 3      */
/* (:376-414), check_gap_errors per entry (FILTER 4), max_number_of_factorizations (:438-442)   */
/* and the refinement loop per entry, in ONE call, nothing leaving HBM in between.  The three   */
/* stage kernels are the ones of the chained entries, one query per candidate; what compares    */
/* candidates with each other is one wave per EST.                                              */
/* ------------------------------------------------------------------------------------------ */
#define PGPU_FLIST_MAX_CANDIDATES 64u   /* candidates of one EST (one lane per list entry); beyond: HOST at stage 0 */
#define PGPU_FLIST_CAP_CANDIDATES  4u   /* detail of HOST at stage 0 for that cap (0 .. 2 are enumeration kinds) */
typedef struct {
  double  complexity_threshold;       /* clean: config->complexity_threshold */
  int32_t suffpref_length_on_est, suffpref_length_for_intron, suffpref_length_on_gen;   /* refine: each in [0, 2^24] */
  int32_t min_intron_length;          /* refine: config->min_intron_length; only compared: any value */
  double  max_coverage_diff;          /* FILTER 1: config->max_coverage_diff, in [0, 1] */
  int32_t max_site_difference;        /* add_if_not_exists: (int) config->max_site_difference, in [0, 2^24] */
  int32_t max_gaplength_diff;         /* FILTER 3: config->max_gapLength_diff, >= -1; -1 switches the filter off */
  int32_t max_number_of_factorizations;   /* :438-442, in [0, 2^24]; 0 switches the rule off.  A negative value is
                                             PGPU_EINVAL: what the reference does with one stays with the caller */
  uint32_t reserved;                  /* 0 */
} pgpu_flist_params;         /* 48 bytes: 0, 8, 12, 16, 20, 24, 32, 36, 40, 44; no padding */
typedef struct {
  uint64_t est_off; uint32_t est_len; /* EST_seq = ests + est_off, est_len bytes, 1 .. 2^31 - 1: est_len stands both for
                                         pext->size - 2 and for strlen(EST) */
  uint32_t first_candidate, n_candidates;   /* the EST's candidates = cands[first_candidate .. + n_candidates), in the
                                               enumeration stage's order (root by root, within a root in list order) */
  uint32_t reserved;                  /* 0 */
} pgpu_flist_query;          /* 24 bytes: 0, 8, 12, 16, 20; no padding */
typedef struct {
  uint8_t  outcome;          /* PGPU_FACT_HOST, PGPU_FACT_EMPTY or PGPU_FACT_DONE */
  uint8_t  stage;            /* where the outcome fell: 0 candidates, 1 clean, 2 select, 3 gaps, 4 refine */
  uint16_t detail;           /* HOST at stage 0: PGPU_FLIST_CAP_CANDIDATES (plan form also: the enumeration kind NONE, CYCLIC,
                                RANGE); at stages 1, 3, 4: 1 a cap (that entry's PGPU_ERANGE), 2 an input that entry's validator
                                refuses.  EMPTY: 0, but at stage 3: 1 every entry dropped by check_gap_errors, 2 more entries
                                left than max_number_of_factorizations.  DONE: 0 */
  uint32_t first_fact;       /* DONE only, else 0: facts[first_fact .. first_fact + n_facts), in flist order */
  uint16_t n_facts;          /* DONE only (>= 1), else 0 */
  uint16_t n_cleaned;        /* the list's length after clean, */
  uint16_t n_listed;         /* after add_if_not_exists, */
  uint16_t n_filtered;       /* and after FILTER 3: each whenever that point was reached, else 0 */
} pgpu_flist_result;         /* 16 bytes: 0, 1, 2, 4, 8, 10, 12, 14 */
#define PGPU_FLIST_DROPPED_FIRST 1u   /* flags bit 0: dropped_first of pgpu_chain_result (the exon is not among the n_exons) */
#define PGPU_FLIST_HEAD_WIDENED  2u   /* bit 1: an equal candidate (res == -2) gave the head its EST_start and GEN_start */
#define PGPU_FLIST_TAIL_WIDENED  4u   /* bit 2: ... the tail its EST_end and GEN_end */
typedef struct {
  uint32_t first_exon;       /* exons[first_exon .. first_exon + n_exons), steps likewise (as pgpu_index_factorizations') */
  uint16_t n_exons;          /* >= 1 */
  uint16_t n_merged;         /* exons check_gap_errors merged into the one before them */
  uint32_t candidate;        /* index, in the call's table, of the candidate the factorization began as */
  uint16_t total_edit;       /* tot_out_edit_distance of check_gap_errors (<= PGPU_GAPS_MAX_ERRORS) */
  uint16_t flags;            /* PGPU_FLIST_* */
} pgpu_flist_fact;           /* 16 bytes: 0, 4, 6, 8, 12, 14 */

/* Per EST, with its candidates c0 .. c(m-1).  clean_candidates is called per root on one growing flist, so the rule is a
 * flat fold in candidate order.
 *  0. m == 0: EMPTY at stage 0.  m > PGPU_FLIST_MAX_CANDIDATES: HOST at stage 0, detail PGPU_FLIST_CAP_CANDIDATES.
 *  1. Every candidate goes through pgpu_index_clean_chains' steps on a query of its own.  A candidate that gets
 *     PGPU_ERANGE (detail 1), or is a query that entry's validator refuses (detail 2: a coordinate outside its string, an
 *     end exon of a list that passes step 1 beginning in front of or ending behind its string), makes the EST HOST at stage
 *     1; the lowest such candidate index decides the detail.  Verdicts 1 .. 7 drop that candidate only.  None left: EMPTY.
 *  2. add_if_not_exists over the survivors (their kept runs [first_kept, first_kept + n_kept) of clean's out_exons), in
 *     candidate order.  to_add is compared with every list entry from the front; res is
 *       - both of one exon (:2053-2066): -2 when GEN_start and GEN_end are equal, else -1 when to_add lies inside the entry
 *         on the genomic sequence (>=, <=), else 1 when the entry lies inside to_add, else 0;
 *       - else relaxed_list_contained(to_add, entry, relaxed_factor_compare, max_site_difference) (src/list.c:320-483):
 *         equal lengths: -2 when every pair compares 0 under cfr_type -2 for the first, -1 for the last and 0 between (two
 *         lists of one exon never get here; a list of one exon against a longer one is 0); unequal lengths: the shorter
 *         list's first exon is looked for along the longer one (cfr_type -2 at the longer one's first exon, 2 behind it),
 *         then both advance together under cfr_type 0, and for the shorter list's last exon 1, or -1 when it meets the
 *         longer list's last; a mismatch is 0; when the shorter list is used up exactly: 1 when to_add is the longer one,
 *         -1 when it is the shorter one.  The loop counts a step even when it ends on a list's end, so a shorter list whose
 *         exons run out of partners is 0.
 *       - relaxed_factor_compare(p1, p2, cfr_type, allowed, l1) (src/est-factorizations.c:1159-1259), p1 always of the
 *         longer list l1 (of to_add for equal lengths): 1 when the two exons do not overlap on the genomic sequence
 *         (strictly apart); cfr_type 0: 0 when both genomic ends differ by at most `allowed`; |cfr_type| 2: the ends agree;
 *         for +2, p1.GEN_start - p2.GEN_start > 20 (max_unconf) is 1, and when it is > 0 with tot = the genomic lengths of
 *         l1's exons in front of the one that begins where p1 does, |p1.GEN_start - p2.GEN_start - tot| < 10 is 1; else 0;
 *         |cfr_type| 1: the starts agree; for +1 the same with p2.GEN_end - p1.GEN_end, tot summed from l1's back, and the
 *         constant 20; whatever matches no branch is 1.
 *     The first entry with res < 0 stops the walk and to_add is not added; when that res is -2 the entry's head takes
 *     EST_start and GEN_start of to_add's head if to_add's EST_start is smaller, and its tail EST_end and GEN_end of
 *     to_add's tail if that EST_end is larger (in place: later compares see the widened entry).  Entries in front of the
 *     stop with res == 1 are removed -- all such entries when nothing stops the walk, and then to_add is appended.  The
 *     list's order is the order of appends, which is candidate order.
 *     FILTER 1: cov = (double)(est_len - (head.EST_start + (est_len - tail.EST_end - 1))) / (double) est_len, int and FP64
 *     as :1262-1273; max_cov over the list from 0.0; an entry goes when max_cov - cov > max_coverage_diff, else when
 *     (max_cov - cov) * (double)(int) est_len > 100.  An entry of one exon with EST_start outside [0, est_len) goes first
 *     (:290-296; clean's verdict 1 lets none arrive).  No product is contracted into an FMA.
 *     FILTER 3, on what FILTER 1 left: g = the sum of EST_start - previous EST_end - 1 over the entry (0 for one exon);
 *     min_gl is folded over the list from -1 by `min_gl == -1 || min_gl > g` -- a minimum that has become -1 (exons that
 *     share an EST byte) is replaced by the next entry's g whatever that is, as :389-392 do; an entry goes when
 *     max_gaplength_diff != -1 and g - min_gl > max_gaplength_diff.  Neither filter can empty the list.
 *  3. Every entry left goes through pgpu_index_gap_chains' steps with its merged ends.  An entry that entry's validator
 *     refuses (detail 2) or PGPU_ERANGE (detail 1): HOST at stage 3, the lowest candidate index deciding.  Verdict 1 drops
 *     the entry.  None left: EMPTY, detail 1.  Then, when max_number_of_factorizations != 0 and more entries are left
 *     than that: EMPTY, detail 2.
 *  4. Every entry left, less the exons gaps merged, goes through pgpu_index_refine_chains' steps with the call's four
 *     settings.  Two adjacent exons not strictly in order (detail 2) or PGPU_ERANGE (detail 1): HOST at stage 4, the lowest
 *     candidate index deciding.  Otherwise DONE: the factorizations in flist order, each with the first-exon rule
 *     (:476-485) applied.
 *  - An outcome never depends on another EST of the call; a candidate a filter or a verdict removed runs the later stages'
 *    trivial queries on a placeholder exon of its own and never reaches a later cap.  The work budget stays with the caller.
 *  - facts, exons and steps of a call are compact: EST order, then list order.  The step bytes are as in
 *    pgpu_index_factorizations. */

/* Index form.  cands: n_cands_total entries, as pgpu_index_candidate_lists writes them (n_pairs and root are not looked at);
 * exons: n_exons_total entries.  out: n results; facts: facts_cap entries; out_exons, out_steps: exons_cap entries;
 * *n_facts, *n_exons: what was written.  One upload, one download.
 *  - PGPU_EINVAL for the whole call only for structure: a null pointer (no message); est_off + est_len > ests_len;
 *    est_len == 0 or > 2^31 - 1; a reserved word != 0 (query, named candidate, parameters); first_candidate + n_candidates
 *    > n_cands_total; a named candidate with n_exons == 0 or first_exon + n_exons > n_exons_total; two queries sharing a
 *    candidate; two candidates sharing an exon; a parameter outside the range stated above; more than 2^31 - 1 queries,
 *    candidates or exons.  A candidate no query names is not looked at.  Whatever concerns the VALUES of the exons is
 *    HOST for that EST.
 *  - PGPU_ENOSPC, with both needed counts in *n_facts and *n_exons and nothing written to out, facts, out_exons or
 *    out_steps, when facts_cap or exons_cap is too small.
 *  - n == 0 is PGPU_OK (both counts 0).  idx may be built or loaded. */
int pgpu_index_factorization_lists(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                   const pgpu_enum_candidate* cands, size_t n_cands_total, const pgpu_factor* exons,
                                   size_t n_exons_total, const pgpu_flist_query* q, size_t n, const pgpu_flist_params* params,
                                   pgpu_flist_result* out, pgpu_flist_fact* facts, size_t facts_cap, pgpu_factor* out_exons,
                                   uint8_t* out_steps, size_t exons_cap, size_t* n_facts, size_t* n_exons);
/* HIP-event time of the whole device part of the calling thread's last pgpu_index_factorization_lists on a context with
 * timing on (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_factorization_lists_kernel_ms(void);

/* Plan form: the candidate lists of the last pgpu_pairing_plan_run_candidate_lists, where they lie; the ESTs are the plan's
 * patterns.  A second branch beside the ladder, as run_candidate_lists is: it needs valid candidate lists, changes nothing
 * of what the plan's other stages hold, and its results stay valid until the next run, run_meg or run_candidate_lists of
 * the plan, or the run of another resident plan; after that fetch_factorization_lists is PGPU_EINVAL with a message.  A
 * record whose enumeration kind is NONE, CYCLIC or RANGE is HOST at stage 0 with detail = the kind.  PGPU_EINVAL (with a
 * message) also for bad parameters.  An empty plan is PGPU_OK.  A rerun gives the same bytes. */
int pgpu_pairing_plan_run_factorization_lists(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_flist_params* params);
/* factorizations and exons of the last run_factorization_lists (either pointer may be null) */
int pgpu_pairing_plan_factorization_list_counts(const pgpu_pairing_plan* plan, uint64_t* n_facts, uint64_t* n_exons);
/* out: n_pat results; PGPU_ENOSPC when facts_cap or exons_cap is smaller than the counts */
int pgpu_pairing_plan_fetch_factorization_lists(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_flist_result* out,
                                                pgpu_flist_fact* facts, size_t facts_cap, pgpu_factor* exons, uint8_t* steps,
                                                size_t exons_cap);
/* HIP-event times of the last run_factorization_lists: k = 0 the whole call, 1 clean_kernel, 2 flist_select_kernel,
 * 3 gaps_kernel, 4 chain_kernel; 0 without timing */
double pgpu_pairing_plan_factorization_lists_ms(const pgpu_pairing_plan* plan, int k);

/* ------------------------------------------------------------------------------------------ */
/* final factorizations -- the factorization stage above, then pgpu_index_tail_chains and      */
/* pgpu_index_small_chains on what it left, in ONE call, nothing leaving HBM in between: for an */
/* EST with exactly one candidate this ends with the factorization as refine_EST_factorizations */
/* (src/factorization-refinement.c:1270-1305) leaves it, with the polyA flags and one verdict   */
/* per EST.  The two stage kernels are the ones of the chained entries; between them one thread */
/* per EST does what a caller of those entries does on the host: take out the exons the tail    */
/* stage removed, build the next query, cut the kept run out of small's list.                   */
/* remove_duplicated_factorizations, add_if_not_exists and ef_remove_factorizations_with_very_  */
/* small_exons compare or filter whole factorizations and stay with the caller.  Nothing in the */
/* library calls these entries yet.                                                             */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t  outcome;       /* PGPU_FACT_HOST / EMPTY / DONE */
  uint8_t  stage;         /* 0-3 as pgpu_fact_result; 4 tail; 5 small */
  uint16_t detail;        /* stages 0-3: pgpu_fact_result's. HOST at 4, 5: 1 a cap, 2 the validator. EMPTY at 4: 1;
                             at 5: small's verdict 1 or 2. DONE: bit 0 = dropped_first */
  uint32_t first_exon;    /* DONE only */
  uint16_t n_exons;       /* DONE only, <= 128 */
  uint16_t n_merged;      /* from gaps, whenever stage 3 said DONE */
  uint32_t total_edit;    /* as pgpu_fact_result */
  uint32_t tail_added;    /* whenever tail answered PGPU_OK, else 0 */
  uint8_t  polyA, polyadenil, recovered;   /* the same */
  uint8_t  refused;       /* HOST at stage 5, detail 1: pgpu_small_result.refused; else 0 */
  uint16_t n_removed;     /* exons step 5 of tail removed */
  uint16_t n_added;       /* exons small inserted */
  uint16_t n_cleaned;     /* n_list - n_kept */
  uint8_t  prefix_added, reserved;
} pgpu_final_result;      /* 32 bytes, no padding: 0,1,2,4,8,10,12,16,20,21,22,23,24,26,28,30,31 */
typedef pgpu_tail_query pgpu_final_query;   /* n_exons == 0: no candidate */

/*  - The stages 0-3, per EST, are those of pgpu_fact_result; an EST that is HOST or EMPTY there keeps that outcome, stage
 *    and detail, and total_edit.  An EST that is DONE at stage 3 goes on, each further stage exactly the chained entry of
 *    that name on a query of its own, est_off the WORKING sequence and orig_off the ORIGINAL one:
 *    4. tail on the refined exons.  What pgpu_index_tail_chains refuses for a whole call is HOST with detail 2 for this
 *       EST: a coordinate that is no byte of what it indexes (the rule of stage 3 lets an end equal to a length pass, this
 *       one does not; nothing known gets such a coordinate as far as stage 3, and the test stays).
 *       PGPU_ERANGE is HOST with detail 1.  Verdict 1 is EMPTY, detail 1.  tail_added, polyA, polyadenil and recovered
 *       are pgpu_tail_result's whenever that status is PGPU_OK, under verdict 1 too, and stay whatever stage 5 says;
 *       n_removed = the query's exons - n_kept under verdict 0, else 0;
 *    5. small, with params->min_intron_length, on the exons tail kept (out_steps bits 0-1 != 3), in their order.  What
 *       pgpu_index_small_chains refuses for a whole call: HOST, detail 2.  PGPU_ERANGE: HOST, detail 1, with `refused`
 *       that entry's code 1 .. 5.  Otherwise n_added, prefix_added and n_cleaned = n_list - n_kept are
 *       pgpu_small_result's; verdict 1 or 2: EMPTY with that detail; verdict 0: DONE, detail bit 0 the dropped_first of
 *       stage 3, and the factorization is the run [first_kept, first_kept + n_kept) of small's list.
 *  - exons and steps of a call are compact, in EST order; only DONE has any.  steps[k] is pgpu_index_small_chains'
 *    out_steps of that exon.  A call never has more than twice the candidates' exons.
 *  - An outcome never depends on another EST of the call: an EST with nothing to do at a stage is given that stage's
 *    trivial query on a placeholder exon of its own -- tail: (0, est_len - 1, 0, 0), which extends nothing, has no polyA
 *    window, is valid, has no affix to recover and no neighbour; small: (0, 0, 0, 0), which has no prefix to search, no
 *    pair, and a last cleaning of one cell (the one banded distance of step 3) whose verdict is ignored.  Beside that cell
 *    neither asks a DP question, and neither can be refused.  An empty pattern of a plan (never DONE) has (0, -1, 0, 0) at
 *    tail, which reads nothing and is verdict 1, unread. */

/* A plan whose patterns are WORKING sequences (polyA/T masked) can hold the ORIGINAL ones of the few patterns where the
 * two differ: orig_pat[0 .. n_orig) names those patterns, strictly ascending, and original k is orig_bytes[orig_first[k]
 * .. orig_first[k + 1]), of exactly the length of pattern orig_pat[k].  The originals lie behind the pattern bytes in the
 * same device allocation, with one offset per pattern into it (a pattern without an original: its own offset); they are
 * not packed and take no part in the pairings.  resident != 0: as pgpu_pairing_plan_create_resident, else as
 * pgpu_pairing_plan_create; those two are this call with n_orig == 0.  PGPU_EINVAL with a message: an index >= n_pat, a
 * list that is not strictly ascending, a length that differs, a null pointer with n_orig > 0. */
int pgpu_pairing_plan_create_with_originals(pgpu_ctx* ctx, const pgpu_index* idx, const char* patterns, const uint64_t* pat_off,
                                            size_t n_pat, int resident, const uint32_t* orig_pat, const uint64_t* orig_first,
                                            const char* orig_bytes, size_t n_orig, pgpu_pairing_plan** plan);

/* Plan form: the answer of the last pgpu_pairing_plan_run_factorizations, where it lies; the ESTs are the plan's patterns
 * and their originals.  The fifth stage of a plan: the factorizations stay fetchable and unchanged; a run of any earlier
 * stage takes the finals with it.  PGPU_EINVAL (with a message): no run_factorizations since the last run of an earlier
 * stage; the results of a resident plan were overwritten by the run of another one; params->reserved != 0; fetch before
 * the run.  params == NULL is a bare PGPU_EINVAL.  An empty plan is PGPU_OK.  A rerun gives the same bytes.  The buffers
 * come from where the MEG stage's do.  The one host wait of the call is its last statement (8 bytes: the exon count). */
int pgpu_pairing_plan_run_final_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_small_params* params);
/* The same run with stages 4 and 5 as pgpu_index_tail_chains_wide and pgpu_index_small_chains_wide answer them: the same
 * fifth stage by the same rules, fetched with pgpu_pairing_plan_fetch_final_factorizations, and the stages above it run
 * on what it leaves.  The results equal the narrow run's except where that one is HOST at stage 4 or 5 with detail 1 for
 * a window the wide caps take.  pgpu_pairing_plan_final_ms reports it: the wide kernels inside the pairs k = 1 and 2. */
int pgpu_pairing_plan_run_final_factorizations_wide(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_small_params* params);
uint64_t pgpu_pairing_plan_final_exons(const pgpu_pairing_plan* plan);   /* exons of the last run_final_factorizations */
/* out: n_pat results; exons, steps: at least final_exons entries (PGPU_ENOSPC when cap is smaller) */
int pgpu_pairing_plan_fetch_final_factorizations(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_final_result* out,
                                                 pgpu_factor* exons, uint8_t* steps, size_t cap);
/* HIP-event times of the last run_final_factorizations: k = 0 the whole call (hand-off kernels and the scan included),
 * 1 tail_kernel, 2 small_kernel; 0 without timing */
double pgpu_pairing_plan_final_ms(const pgpu_pairing_plan* plan, int k);

/* Index form: candidate -> clean -> gaps -> refine -> tail -> small for a caller that holds candidates.  One query = one
 * EST: the fields of pgpu_tail_query, where n_exons == 0 means "no candidate" (HOST at stage 0, detail PGPU_CAND_NONE;
 * first_exon is then not looked at).  out: n results; out_exons, out_steps: cap entries; *n_out: exons written, never more
 * than 2 * n_exons_total.  One upload, one download; synchronous and batched like the other pgpu_index_* queries.
 *  - PGPU_EINVAL for the whole call only for structure: what pgpu_index_factorizations lists, orig_off + est_len >
 *    ests_len, and small_params == NULL (no message) or small_params->reserved != 0.  Whatever concerns the VALUES of the
 *    exons is HOST for that query, exactly as in the plan form.
 *  - PGPU_ENOSPC, with the needed count in *n_out and nothing written to out, out_exons or out_steps, when cap is too small.
 *  - n == 0 is PGPU_OK (*n_out = 0).  idx may be built or loaded; the classification tables are built on first use as for
 *    pgpu_index_small_exons. */
int pgpu_index_final_factorizations(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                    const pgpu_factor* exons, size_t n_exons_total, const pgpu_final_query* q, size_t n,
                                    const pgpu_fact_params* params, const pgpu_small_params* small_params,
                                    pgpu_final_result* out, pgpu_factor* out_exons, uint8_t* out_steps, size_t cap, size_t* n_out);
/* HIP-event time of the whole device part (both drivers) of the calling thread's last pgpu_index_final_factorizations on
 * a context with timing on (as pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_index_final_factorizations_kernel_ms(void);
/* pgpu_index_final_factorizations with stages 4 and 5 as the two wide chained entries answer them; everything else, the
 * _kernel_ms getter included, is that entry's */
int pgpu_index_final_factorizations_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                         const pgpu_factor* exons, size_t n_exons_total, const pgpu_final_query* q, size_t n,
                                         const pgpu_fact_params* params, const pgpu_small_params* small_params,
                                         pgpu_final_result* out, pgpu_factor* out_exons, uint8_t* out_steps, size_t cap,
                                         size_t* n_out);

/* ------------------------------------------------------------------------------------------ */
/* units -- from the finals of the patterns to est-fact's answer per INPUT EST: a unit is an   */
/* input EST with its reverse-complement sibling (src/main-est-fact.c:249-291: the forward      */
/* strand first, the sibling only when the forward one has no factorization).  Per unit one     */
/* verdict, and for an ALIGNED unit the exact bytes of the group est-fact writes into its packed */
/* records (include/pintron_records.h; pintron_amd/host/ef_estfact.c:                            */
/* ef_write_factorization_records, the selection rules of src/io-multifasta.c:187-241), after    */
/* remove_factorizations_with_very_small_exons (src/factorization-refinement.c:84-111).  A caller */
/* of the chain copies bytes for every settled unit and runs its own path for the HOST ones.     */
/* Nothing in the library calls these entries yet.                                              */
/* ------------------------------------------------------------------------------------------ */
#define PGPU_UNIT_NO_SIBLING 0xffffffffu
#define PGPU_UNIT_FWD_SUFF_POLYA 1u   /* info->suff_polyA_length != -1 of the forward sequence */
#define PGPU_UNIT_REV_SUFF_POLYA 2u   /* ... of the sibling as prepared (ef_copy_and_reverse)   */
typedef struct {
  uint32_t est_index;       /* position of the EST in ests.txt: copied into the group, any value */
  uint32_t fwd, rev;        /* pattern indices; rev == PGPU_UNIT_NO_SIBLING: a fixed-strand EST */
  uint32_t flags;           /* PGPU_UNIT_*_SUFF_POLYA */
} pgpu_unit_query;          /* 16 bytes */
typedef struct {
  int32_t pref_N_length;    /* of the genomic sequence (ef_seq.pref_N_length), in [0, 2^30] */
  uint8_t retain_externals; /* 0 or 1 */
  uint8_t reserved[3];
} pgpu_unit_params;         /* 8 bytes */
#define PGPU_UNIT_HOST      0u   /* the caller runs its own path for this EST */
#define PGPU_UNIT_UNALIGNED 1u   /* no factorization on either strand: no group, no entry of processed-ests.txt */
#define PGPU_UNIT_ALIGNED   2u   /* blob[first_byte .. first_byte + n_bytes) is the EST's group */
typedef struct {
  uint8_t  verdict, strand;   /* strand: the pattern that decided (0 fwd, 1 rev) */
  uint8_t  reason;            /* of that pattern: 0 its final outcome as it stands, 1 a very small exon, 2 an empty graph */
  uint8_t  n_factorizations;  /* ALIGNED: 0 or 1, else 0 */
  uint32_t pattern;           /* index of the pattern that decided */
  uint64_t first_byte;        /* ALIGNED only, else 0 */
  uint32_t n_bytes, reserved; /* n_bytes: ALIGNED only, else 0 */
} pgpu_unit_result;         /* 24 bytes: 0, 1, 2, 3, 4, 8, 16, 20 */

/*  - Per pattern, from its pgpu_final_result, its exons, and whether its MEG is empty:
 *      ALIGNED  outcome DONE and every exon has EST_end + 1 - EST_start > 2 (_UB_VERY_SMALL_EXON_LENGTH_; the difference
 *               in the reference's int arithmetic, computed here in 64 bits);
 *      NONE     (no factorization) outcome EMPTY at any stage (reason 0); DONE with a very small exon (reason 1: the
 *               one factorization is removed and the list is empty); or (HOST, stage 0, detail PGPU_CAND_NOT_PATH) with
 *               an empty graph (reason 2): source and sink without an edge, whose one-vertex embeddings become
 *               one-factor factorizations that clean_candidates drops (src/est-factorizations.c:2111-2125).  The
 *               empty-graph bit is looked at in this last case only;
 *      HOST     everything else (reason 0).
 *    The caller's budget and max_number_of_factorizations cannot matter: a path's `work` is at most 128 units against a
 *    budget of at least 10^6, and one factorization never exceeds a limit >= 1 (0 means no limit).
 *  - Per unit: fwd ALIGNED -> ALIGNED on strand 0, the sibling is never looked at; fwd HOST -> HOST on strand 0; fwd
 *    NONE: no sibling -> UNALIGNED (strand 0, the forward pattern and its reason); else the sibling decides (strand 1, its
 *    index and its reason): ALIGNED -> ALIGNED, NONE -> UNALIGNED, HOST -> HOST.
 *  - The group of an ALIGNED unit: u32 est_index, u32 n_factorizations, then per factorization u8 polya, u8 polyad,
 *    u16 n_exons and the exons as four i32 each: EST_start + 1, EST_end + 1, pref_N_length + GEN_start + 1,
 *    pref_N_length + GEN_end + 1, the additions done in uint32_t.  retain_externals != 0: every exon, with the final
 *    result's polyA and polyadenil.  retain_externals == 0: the factorization is written only when n > 2 || (n == 2 && the
 *    deciding strand has a polyA suffix); both flags are 0; the first exon is dropped, and the last one unless that strand
 *    has a polyA suffix; a factorization that is not written leaves a group of 8 bytes with n_factorizations == 0.
 *  - UNALIGNED and HOST units have no bytes.  The blob is compact and in UNIT order, whatever the pattern order: a call
 *    whose units are all settled produces est-fact's blob for those ESTs byte for byte.  Every offset is a multiple of 4. */

/* The form without a plan: fetched or hand-made finals, no index.  res: n_pat results; exons: n_exons_total entries, the
 * ones res[].first_exon index; empty_graph: a byte per pattern (0 or not), or NULL = none is empty; q: n units; out: n
 * results; blob: blob_cap bytes; *blob_len: bytes written.  One upload, one download; synchronous.
 *  - PGPU_EINVAL for the whole call, for structure only: a null pointer (no message); fwd >= n_pat; rev >= n_pat and not
 *    PGPU_UNIT_NO_SIBLING; fwd == rev; a pattern named by two units; flag bits beyond 0-1; reserved != 0;
 *    retain_externals > 1; pref_N_length outside [0, 2^30]; an outcome above 2; a DONE result with n_exons == 0,
 *    n_exons > 128 or first_exon + n_exons > n_exons_total; more than 2^31 - 1 units or patterns.
 *  - PGPU_ENOSPC, with the needed size in *blob_len and nothing written to out or blob, when blob_cap is too small.
 *  - n == 0 is PGPU_OK (*blob_len = 0). */
int pgpu_unit_records(pgpu_ctx* ctx, const pgpu_final_result* res, size_t n_pat, const pgpu_factor* exons, size_t n_exons_total,
                      const uint8_t* empty_graph, const pgpu_unit_query* q, size_t n, const pgpu_unit_params* params,
                      pgpu_unit_result* out, void* blob, size_t blob_cap, size_t* blob_len);
/* HIP-event time of the kernels of the calling thread's last pgpu_unit_records on a context with timing on (as
 * pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_unit_records_kernel_ms(void);

/* Plan form: the finals of the last pgpu_pairing_plan_run_final_factorizations, where they lie, and the empty-graph bit
 * from each pattern's MEG record header in HBM (an unflagged record with n_vertices == 2 and n_edges == 0).  The sixth
 * stage of a plan: the finals stay fetchable and unchanged; a run of any earlier stage takes the units with it.
 * PGPU_EINVAL (with a message): what the form above refuses in q and params; no run_final_factorizations since the last
 * run of an earlier stage; the results of a resident plan were overwritten by the run of another one; fetch before the
 * run.  A null pointer is a bare PGPU_EINVAL (q may be null when n_units == 0).  An empty plan is PGPU_OK.  A rerun gives
 * the same bytes.  The buffers come from where the MEG stage's do, in a slot of the stage's own.  The one host wait of
 * the call is its last statement (8 bytes: the byte total). */
int pgpu_pairing_plan_run_units(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_unit_query* q, size_t n_units,
                                const pgpu_unit_params* params);
uint64_t pgpu_pairing_plan_unit_bytes(const pgpu_pairing_plan* plan);   /* bytes of the blob of the last run_units */
/* out: as many results as the last run_units had units; blob: at least unit_bytes bytes (PGPU_ENOSPC when cap is smaller) */
int pgpu_pairing_plan_fetch_units(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_unit_result* out, void* blob, size_t cap);
/* HIP-event time of the last run_units (count + scan + write); 0 without timing */
double pgpu_pairing_plan_units_ms(const pgpu_pairing_plan* plan);

/* ------------------------------------------------------------------------------------------ */
/* texts -- from a unit's group in the packed records to est-fact's two text files: the lines   */
/* of raw-multifasta-out.txt (write_multifasta_output, src/io-multifasta.c:187-229; on the host */
/* side ef_raw_text_from_records, pintron_amd/host/ef_records.c) and the entry of               */
/* processed-ests.txt (ef_write_single_est_info).  Everything but a few decimal numbers is a   */
/* substring of a sequence that lies in HBM.  Nothing in the library calls these entries yet.   */
/* ------------------------------------------------------------------------------------------ */
#define PGPU_TEXT_MAX_UNIT_BYTES (1u << 24)
#define PGPU_TEXT_NONE 0u   /* the unit is not ALIGNED: no bytes in either blob */
#define PGPU_TEXT_DONE 1u   /* both texts are written */
#define PGPU_TEXT_HOST 2u   /* raw(u) or pests(u) is longer than PGPU_TEXT_MAX_UNIT_BYTES: no bytes, the caller prints this EST */
typedef struct {
  uint64_t raw_first, pests_first;   /* DONE only, else 0: where the unit's texts begin in the two blobs */
  uint32_t raw_bytes, pests_bytes;   /* DONE only, else 0 */
  uint8_t  verdict;                  /* PGPU_TEXT_* */
  uint8_t  reserved[7];
} pgpu_text_result;         /* 32 bytes */

/* The rule.  For an ALIGNED unit u: H is its header bytes (ef_seq.id, the same for both strands: ef_copy_and_reverse), S
 * the original sequence of the pattern that decided (pgpu_unit_result.pattern), sl bytes, G the original genomic sequence
 * (ef_seq.original_seq, N prefix included), gl bytes, and the group is blob[first_byte .. first_byte + n_bytes).
 *    pests(u) = ">" H "\n" S "\n"
 *    raw(u)   = for each factorization of the group, in order:
 *                 ">" H "\n#polya=" d(polya) "\n#polyad=" d(polyad) "\n", then per exon
 *                 d(est_start) " " d(est_end) " " d(gen_start) " " d(gen_end) " " E " " X "\n"
 *  - d is printf("%d") of the stored value: u8 for the flags, i32 for the four numbers, "-" for negatives,
 *    "-2147483648" for INT_MIN.
 *  - E is the stretch of S: with a = est_start and b = est_end as 64-bit integers it is empty unless
 *    a >= 1 && a <= sl + 1 && b >= a; otherwise it is S[a-1 .. a-1+n) with n = min(b + 1 - a, sl - (a - 1)).
 *    X is the same rule on G with gl.  This is ef_raw_text_from_records' rule stated in 64 bits, so that no input is
 *    undefined; for the records the chain makes it equals ef_write_multifasta_output.
 *  - A group of 8 bytes (n_factorizations == 0) has an empty raw and a full pests.  Headers are copied as they are,
 *    whatever bytes they hold.
 *  - Per unit one pgpu_text_result: NONE for a unit that is not ALIGNED; HOST when raw(u) or pests(u) is longer than
 *    PGPU_TEXT_MAX_UNIT_BYTES (the count formed in 64 bits); DONE otherwise.  Both blobs are compact and in UNIT order: a
 *    call whose units are all settled produces est-fact's two files for those ESTs byte for byte. */

/* The original genomic sequence in HBM (len bytes, copied).  len == 0 or a null pointer: PGPU_EINVAL. */
typedef struct pgpu_text_source pgpu_text_source;
int pgpu_text_source_create(pgpu_ctx* ctx, const char* genomic_original, size_t len, pgpu_text_source** src);
int pgpu_text_source_destroy(pgpu_ctx* ctx, pgpu_text_source* src);

/* The form without a plan: fetched or host-made records, no index, any well-formed group (several factorizations too: the
 * device twin of ef_raw_text_from_records).  units: n results of the unit stage; blob: the groups they name; headers:
 * headers_len bytes, hdr_first: n + 1 offsets, unit i's header is headers[hdr_first[i] .. hdr_first[i+1]); seqs: seqs_len
 * bytes, seq_first: n_pat + 1 offsets, one sequence per pattern; genomic: genomic_len bytes; out: n results; raw / pests:
 * raw_cap / pests_cap bytes; *raw_len, *pests_len: bytes written.  One upload, one download; synchronous.
 *  - PGPU_EINVAL for the whole call, for structure only: a null pointer (no message); offsets that do not ascend or that
 *    pass their length; a verdict above 2; an ALIGNED unit whose pattern >= n_pat, whose first_byte + n_bytes > blob_len,
 *    whose first_byte or n_bytes is no multiple of 4, or whose factorization headers do not add up to exactly n_bytes;
 *    more than 2^31 - 1 units or patterns.
 *  - PGPU_ENOSPC, with both needed sizes in *raw_len and *pests_len and nothing written to out, raw or pests, when a cap
 *    is too small.
 *  - n == 0 is PGPU_OK (both lengths 0). */
int pgpu_unit_texts(pgpu_ctx* ctx, const pgpu_unit_result* units, size_t n, const void* blob, size_t blob_len,
                    const char* headers, size_t headers_len, const uint64_t* hdr_first,
                    const char* seqs, size_t seqs_len, const uint64_t* seq_first, size_t n_pat,
                    const char* genomic, size_t genomic_len, pgpu_text_result* out,
                    void* raw, size_t raw_cap, size_t* raw_len, void* pests, size_t pests_cap, size_t* pests_len);
/* HIP-event time of the kernels of the calling thread's last pgpu_unit_texts on a context with timing on (as
 * pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_unit_texts_kernel_ms(void);

/* Plan form: the units and the blob of the last pgpu_pairing_plan_run_units, where they lie; the sequences are the plan's
 * originals where a pattern has one, else its own bytes, their lengths from the pattern offsets; G is `src`.  headers /
 * hdr_first: n_units + 1 offsets for the units of that run_units, uploaded at every call.  The seventh stage of a plan:
 * units and finals stay fetchable and unchanged; a run of any earlier stage takes the texts with it.
 * PGPU_EINVAL (with a message): bad header offsets; a source made on another context; no run_units since the last run of
 * an earlier stage; the results of a resident plan were overwritten by the run of another one; fetch before the run.  A
 * null pointer is a bare PGPU_EINVAL (headers may be null when headers_len == 0, hdr_first when the run had no units).  An empty plan or a run of zero units is
 * PGPU_OK.  A rerun gives the same bytes.  The buffers come from where the MEG stage's do, in slots of the stage's own.
 * The one host wait of the call is for the two byte totals that size the blobs: the write pass is still queued when the
 * call returns, and fetch_texts (or texts_ms) waits for it. */
int pgpu_pairing_plan_run_texts(pgpu_ctx* ctx, pgpu_pairing_plan* plan, const pgpu_text_source* src, const char* headers,
                                size_t headers_len, const uint64_t* hdr_first);
/* bytes of a blob of the last run_texts: which == 0 raw, 1 pests, anything else 0 */
uint64_t pgpu_pairing_plan_text_bytes(const pgpu_pairing_plan* plan, int which);
/* out: as many results as the last run_units had units; PGPU_ENOSPC when a cap is smaller than its text_bytes */
int pgpu_pairing_plan_fetch_texts(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_text_result* out, void* raw, size_t raw_cap,
                                  void* pests, size_t pests_cap);
/* HIP-event time of the last run_texts (count + scans + write; waits for the write pass); 0 without timing */
double pgpu_pairing_plan_texts_ms(pgpu_pairing_plan* plan);
/* the write pass alone, the same way */
double pgpu_pairing_plan_texts_write_ms(pgpu_pairing_plan* plan);

/* ------------------------------------------------------------------------------------------ */
/* sides -- from a unit's MEG records to est-fact's three side files: the entries of megs.txt   */
/* and processed-megs.txt and the lines of meg-edges.txt (report_meg and the writes behind it,  */
/* src/compute-est-fact.c:73-88, 240-268; pintron_amd/host/ef_estfact.c: ef_compute_est_fact).  */
/* A MEG record ends with meg_write's text and the meg-edges.txt lines of its graph, so the     */
/* stage is the rule for which entries an input EST gets, and copying.  processed-megs-info.txt */
/* holds per-EST microseconds and is not part of this stage.  Nothing in the library calls      */
/* these entries yet.                                                                           */
/* ------------------------------------------------------------------------------------------ */
#define PGPU_SIDE_MAX_UNIT_BYTES (1u << 24)
#define PGPU_SIDE_NONE 0u   /* the unit is HOST: no bytes in any blob */
#define PGPU_SIDE_DONE 1u   /* the three texts are written */
#define PGPU_SIDE_HOST 2u   /* one of the three texts is longer than PGPU_SIDE_MAX_UNIT_BYTES, or (below) the unit is not one
                               the rule covers: no bytes, the caller prints this EST */
typedef struct {
  uint64_t megs_first, pmegs_first, edges_first;   /* DONE only, else 0: where the unit's texts begin in the three blobs */
  uint32_t megs_bytes, pmegs_bytes, edges_bytes;   /* DONE only, else 0 */
  uint8_t  verdict;                                /* PGPU_SIDE_* */
  uint8_t  reserved[3];
} pgpu_side_result;         /* 40 bytes */

/* The rule.  For a unit u with forward pattern f = q.fwd and sibling r = q.rev: H is the unit's header bytes (ef_seq.id,
 * the same for both strands: ef_copy_and_reverse), S_x the original sequence of pattern x, M_x the meg_text_len bytes of
 * pattern x's MEG record (the record of the FIRST attempt: a settled unit was never retried), X_x the edges_text_len bytes
 * behind them, SEP = "\n\n***********\n\n" (15 bytes), and E(x) = ">" H "\n" S_x "\n" M_x.
 *    unit verdict, strand         megs(u)                pmegs(u)   edges(u)
 *    ALIGNED, 0                   SEP E(f)               E(f)       ">" H "\n" X_f
 *    ALIGNED, 1                   SEP E(f) SEP E(r)      E(r)       ">" H "\n" X_r
 *    UNALIGNED, 0 (no sibling)    SEP E(f)               empty      empty
 *    UNALIGNED, 1                 SEP E(f) SEP E(r)      empty      empty
 *    HOST                         no bytes               no bytes   no bytes
 *  - An UNALIGNED unit does have an entry of megs.txt (in this the stage differs from the text stage).  A HOST unit has no
 *    bytes because the host's own path may build that EST's MEG again with a longer factor.
 *  - Per unit one pgpu_side_result: NONE for a HOST unit; HOST when megs(u), pmegs(u) or edges(u) is longer than
 *    PGPU_SIDE_MAX_UNIT_BYTES (the count formed in 64 bits), and for an UNALIGNED unit of strand 0 that has a sibling
 *    (est-fact never leaves such an EST: it goes on to the sibling); DONE otherwise.  The three blobs are compact and in
 *    UNIT order, whatever the pattern order: a call whose units are all settled produces est-fact's three files for those
 *    ESTs byte for byte. */

/* The form without a plan: fetched or host-made records.  q / units: the n queries and results of the unit stage; recs:
 * recs_len bytes and rec_first: n_pat + 1 offsets, as pgpu_pairing_plan_fetch_meg gives them; headers: headers_len bytes,
 * hdr_first: n + 1 offsets, unit i's header is headers[hdr_first[i] .. hdr_first[i+1]); seqs: seqs_len bytes, seq_first:
 * n_pat + 1 offsets, one (original) sequence per pattern; out: n results; megs / pmegs / edges: their caps in bytes;
 * lens[0 .. 3): bytes written to the three.  One upload, one download; synchronous.
 *  - PGPU_EINVAL for the whole call, for structure only: a null pointer (no message); offsets that do not ascend or that
 *    pass their length; a rec_first that is no multiple of 4; a verdict above 2 or a strand above 1; fwd or rev >= n_pat
 *    (rev may be PGPU_UNIT_NO_SIBLING); strand 1 on a unit without a sibling; units[i].pattern other than the query's
 *    pattern of that strand; a settled unit (not HOST) naming a record -- f, and r too on strand 1 -- that is flagged
 *    (PGPU_MEG_TOO_COMPLEX, PGPU_MEG_UNAVAILABLE), or whose graph part, 8 bytes of lengths and two texts pass
 *    rec_first[x + 1]; more than 2^31 - 1 units or patterns.
 *  - PGPU_ENOSPC, with the three needed sizes in lens and nothing written to out, megs, pmegs or edges, when a cap is
 *    too small.
 *  - n == 0 is PGPU_OK (all three lengths 0). */
int pgpu_unit_sides(pgpu_ctx* ctx, const pgpu_unit_query* q, const pgpu_unit_result* units, size_t n,
                    const void* recs, size_t recs_len, const uint64_t* rec_first, size_t n_pat,
                    const char* headers, size_t headers_len, const uint64_t* hdr_first,
                    const char* seqs, size_t seqs_len, const uint64_t* seq_first,
                    pgpu_side_result* out, void* megs, size_t megs_cap, void* pmegs, size_t pmegs_cap,
                    void* edges, size_t edges_cap, size_t lens[3]);
/* HIP-event time of the kernels of the calling thread's last pgpu_unit_sides on a context with timing on (as
 * pgpu_index_find_kernel_ms); 0 without timing */
double pgpu_unit_sides_kernel_ms(void);

/* Plan form, the eighth stage of a plan: no arguments, because everything lies in HBM already -- the records and their
 * offsets of the last run_meg, the queries and results of the last run_units, the headers and their offsets where the last
 * run_texts left them (so they do not travel a second time: this is why the stage stands above the texts and not beside
 * them), and the plan's originals (a pattern's own bytes where it has none).  A PGPU_TEXT_HOST verdict of the text stage
 * does not matter to this one.  Here a settled unit that names a record which is flagged or does not add up is
 * PGPU_SIDE_HOST (the form without a plan refuses it).  Texts, units and finals stay fetchable and unchanged; a run of any
 * earlier stage, run_texts included, takes the sides with it.  PGPU_EINVAL (with a message): no run_texts since the last
 * run of an earlier stage; the results of a resident plan were overwritten by the run of another one; fetch before the
 * run.  A null pointer is a bare PGPU_EINVAL.  An empty plan or a run of zero units is PGPU_OK.  A rerun gives the same
 * bytes.  The one host wait of the call is for the three byte totals that size the blobs: the write pass is still queued
 * when the call returns, and fetch_sides (or sides_ms) waits for it. */
int pgpu_pairing_plan_run_sides(pgpu_ctx* ctx, pgpu_pairing_plan* plan);
/* bytes of a blob of the last run_sides: which == 0 megs, 1 pmegs, 2 edges, anything else 0 */
uint64_t pgpu_pairing_plan_side_bytes(const pgpu_pairing_plan* plan, int which);
/* out: as many results as the last run_units had units; PGPU_ENOSPC when a cap is smaller than its side_bytes */
int pgpu_pairing_plan_fetch_sides(pgpu_ctx* ctx, pgpu_pairing_plan* plan, pgpu_side_result* out, void* megs, size_t megs_cap,
                                  void* pmegs, size_t pmegs_cap, void* edges, size_t edges_cap);
/* HIP-event time of the last run_sides (count + scans + write; waits for the write pass); 0 without timing */
double pgpu_pairing_plan_sides_ms(pgpu_pairing_plan* plan);
/* the write pass alone, the same way */
double pgpu_pairing_plan_sides_write_ms(pgpu_pairing_plan* plan);

/* page-locked host memory for the buffers handed to the fetch calls (a pageable destination
 * makes the runtime stage the copy); plain malloc'ed memory works too, slower */
int pgpu_host_alloc(pgpu_ctx* ctx, size_t bytes, void** out);
int pgpu_host_free(pgpu_ctx* ctx, void* p);

/* ------------------------------------------------------------------------------------------ */
/* gather -- the single exchange of the EST-sharded run (one process per GPU):    */
/* each rank hands in the bytes it produced (packed factorization records, or the text of an   */
/* output file), rank 0 receives them in rank order = input order.  RCCL point-to-point over   */
/* xGMI; the library loads RCCL on first use.  The reference has no counterpart: its est-fact  */
/* is one process (src/main-est-fact.c:249-291 is the loop that is sharded here).              */
/* ------------------------------------------------------------------------------------------ */
typedef struct pgpu_comm pgpu_comm;
typedef struct { char bytes[128]; } pgpu_comm_id;     /* = ncclUniqueId */
/* rank 0 makes the id and passes it to the other ranks by any means (est-fact: a file) */
int pgpu_comm_unique_id(pgpu_ctx* ctx, pgpu_comm_id* id);
int pgpu_comm_init(pgpu_ctx* ctx, int rank, int world, const pgpu_comm_id* id, pgpu_comm** comm);
/* send/send_bytes: this rank's payload (host memory).  counts: `world` entries, filled on every
 * rank.  recv/recv_cap: rank 0 only, receives sum(counts) bytes.  Collective: all ranks call it. */
int pgpu_gather(pgpu_ctx* ctx, pgpu_comm* comm, const void* send, uint64_t send_bytes,
                void* recv, uint64_t recv_cap, uint64_t* counts);
/* fixed-size all-gather: every rank contributes `bytes` bytes (host memory) and receives world x bytes
 * in rank order.  est-fact --gpus=N uses it once per run for the ranks' status word and output sizes:
 * a rank that failed is seen by all before any payload moves. */
int pgpu_allgather(pgpu_ctx* ctx, pgpu_comm* comm, const void* send, uint64_t bytes, void* recv);
int pgpu_comm_destroy(pgpu_ctx* ctx, pgpu_comm* comm);

/* ------------------------------------------------------------------------------------------ */
/* batched dynamic programs                                                                   */
/* ------------------------------------------------------------------------------------------ */
enum pgpu_dp_kind {
  /* compute_alignment (src/compute-alignments.c:39-207): a = EST string, b = genomic string.
   * v[0]=score v[1]=alignment_dim; str[0], str[1] = offsets of EST_alignment and GEN_alignment in
   * the output string buffer (both NUL-terminated).
   * p0 = 1 / 2 (optional): the alignment is handle_endpoints' of a FIRST / LAST exon
   * (src/est-factorizations.c:2145,2204); p1, p2 = the complexity threshold's double bits.  The library may then
   * answer, beside the alignment, the exon check (KBAND with tail = 1) of the exon as that routine is going to trim
   * it (:2163-2196, :2231-2296): v[4] bit 3 set = answered, for the sub-operands v[2], v[3] (first exon: characters
   * of a / of b trimmed away at the front; last exon: characters of a / of b kept) with the bound v[4] >> 8;
   * v[4] bit 0 = K_band_edit_distance's verdict, bits 1-2 = the two dust comparisons.  The caller files the answer
   * under the question those values define and still does its own trimming: the extra answer saves a request when
   * the two agree, and is never used when they do not. */
  PGPU_DP_ALIGN = 0,
  /* compute_gap_alignment (src/refine-intron.c:560-890): a = EST window, b = genomic window.
   * v[0]=gap_alignment_dim v[1]=factor_cut v[2]=intron_start v[3]=intron_end
   * v[4]=intron_start_on_align v[5]=intron_end_on_align; strings at str[0], str[1] offsets. */
  PGPU_DP_GAP = 1,
  /* Levenshtein distance without N wildcard = last cell of edit_distance (src/refine.c:50-83)
   * = compute_edit_distance (src/compute-alignments.c:240-249).  v[0]=distance. */
  PGPU_DP_ED = 2,
  /* K_band_edit_distance (src/compute-alignments.c:319-453): p0 = upper_bound.
   * v[0]=returned bool, v[1]=*edit.
   * tail = 1 ("exon check", a = the exon on the genomic sequence, b = on the EST): also the two comparisons of
   * clean_low_complexity_exons_2 (src/est-factorizations.c:1687-1691) for this exon -- dustScore
   * (src/exon-complexity.c:50-78) of each operand against the threshold whose IEEE double bits are p1 (low word)
   * and p2 (high word): v[2] bit 0 = dust(a) > threshold, bit 1 = dust(b) > threshold.  The score is computed in
   * FP64 in the reference's operation order (integer sum, x 10.0, / (length - 2), / length). */
  PGPU_DP_KBAND = 3,
  /* find_longest_common_factor_dp (src/factorization-refinement.c:255-316): a = s1, b = s2.
   * v[0]=len v[1]=occ1 v[2]=occ2. */
  PGPU_DP_LCF = 4,
  /* general_refine_borders (src/refine.c:105-192): a = p, b = t, p0=min_p_cut p1=max_p_cut
   * p2=max_errs, tail = number (0..2) of valid bytes that follow t in its buffer (the reference
   * reads t[len_t], t[len_t+1] in getBursetFrequency_adaptor).
   * v[0]=returned bool v[1]=out_offset_p v[2]=out_offset_t1 v[3]=out_offset_t2 v[4]=edit. */
  PGPU_DP_BORDERS = 5,
  /* find_longest_affix (src/factorization-refinement.c:1136-1173): a = est, b = genomic.
   * v[0]=valid_cut v[1]=est cut v[2]=genomic cut. */
  PGPU_DP_AFFIX = 6,
  PGPU_DP_NKINDS = 7
};

#define PGPU_JOB_A_GENOMIC 1u   /* a_off indexes the resident genomic of the index, not the arena */
#define PGPU_JOB_B_GENOMIC 2u   /* same for b_off */

typedef struct {
  uint32_t kind;            /* enum pgpu_dp_kind */
  uint32_t flags;           /* PGPU_JOB_* */
  uint64_t a_off, b_off;    /* byte offsets of the operands (arena or genomic) */
  uint32_t a_len, b_len;
  uint32_t p0, p1, p2;      /* kind-specific parameters */
  uint32_t tail;            /* BORDERS only */
} pgpu_dp_job;              /* 48 bytes */

typedef struct {
  int32_t status;           /* PGPU_OK or PGPU_ERANGE for this job */
  int32_t v[6];             /* kind-specific, see enum */
  int32_t pad;
  uint64_t str[2];          /* ALIGN/GAP: offsets of the two alignment strings */
} pgpu_dp_result;           /* 48 bytes */

/* limits (per job); larger jobs get status PGPU_ERANGE */
#define PGPU_MAX_ROWS_LEV     65536u  /* ALIGN, AFFIX: a_len; ED, KBAND: min(a_len,b_len) (beyond 4096 rows
                                        one wave sweeps the matrix in strips of 4096 rows) */
#define PGPU_MAX_ROWS_BORDERS 4096u  /* BORDERS: a_len of the fast kernels; up to PGPU_MAX_ROWS_LEV a slow
                                        anti-diagonal kernel over HBM answers instead of refusing */
#define PGPU_MAX_ROWS_GAP     2048u  /* GAP: a_len of the fast kernels; larger windows take the slow kernel */
#define PGPU_MAX_GAP_SIDE    16000u  /* GAP: a_len and b_len */
#define PGPU_MAX_GAP_CELLS (1ull << 27)   /* GAP: (a_len+1)*(b_len+1), one direction byte per cell */
#define PGPU_MAX_COLS      1048576u

/* A plan holds a batch of jobs resident in HBM: operands, sorted job table, workspaces, results.
 * create = sort by kernel/size + one upload; launch = enqueue every kernel of the batch (fanned
 * over the context's streams, asynchronous) and, behind them, the download of results and
 * alignment strings; sync = wait; fetch = hand the results out in the caller's job order.
 * idx may be NULL when no job uses PGPU_JOB_*_GENOMIC.  One plan per context at a time is the
 * fast path (its device and pinned buffers are the context's own). */
int pgpu_dp_plan_create(pgpu_ctx* ctx, const pgpu_index* idx,
                        const pgpu_dp_job* jobs, size_t n_jobs,
                        const char* arena, size_t arena_len, pgpu_dp_plan** plan);
/* The same for a batch assembled from several producers (the host program's worker threads): the
 * jobs of a part address that part's arena; results come back in the order of the parts, jobs of
 * part 0 first.  Nothing is copied on the caller's side: the library gathers jobs and arenas
 * straight into its pinned upload image. */
typedef struct { const pgpu_dp_job* jobs; size_t n_jobs; const char* arena; size_t arena_len; } pgpu_dp_part;
int pgpu_dp_plan_create_parts(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_dp_part* parts, size_t n_parts,
                              pgpu_dp_plan** plan);
int pgpu_dp_plan_launch(pgpu_ctx* ctx, pgpu_dp_plan* plan);
int pgpu_dp_plan_sync(pgpu_ctx* ctx, pgpu_dp_plan* plan);
/* bytes the alignment strings of this plan need in fetch's `strings` buffer */
size_t pgpu_dp_plan_string_bytes(const pgpu_dp_plan* plan);
int pgpu_dp_plan_fetch(pgpu_ctx* ctx, pgpu_dp_plan* plan, pgpu_dp_result* results,
                       char* strings, size_t strings_cap);
/* copies the result table (n_jobs * sizeof(pgpu_dp_result), caller order) into DEVICE memory the
 * caller owns (e.g. a buffer handed to an RCCL gather); waits for the plan first (the table is
 * completed on the host: the LCF answers are decoded there from the keys the kernel leaves);
 * returns after the copy has completed */
int pgpu_dp_plan_results_to_device(pgpu_ctx* ctx, pgpu_dp_plan* plan, void* device_dst, size_t cap);
int pgpu_dp_plan_destroy(pgpu_ctx* ctx, pgpu_dp_plan* plan);

/* measurement hooks (bench.py): DP cells of the plan per kind with the reference's own loop
 * bounds, algorithmic HBM bytes per kind, and the duration of the last
 * launch of each kind's kernels measured with HIP events on the context's stream. */
uint64_t pgpu_dp_plan_cells(const pgpu_dp_plan* plan, int kind);
uint64_t pgpu_dp_plan_algo_bytes(const pgpu_dp_plan* plan, int kind);
double   pgpu_dp_plan_kernel_ms(const pgpu_dp_plan* plan, int kind);
uint64_t pgpu_dp_plan_launches(const pgpu_dp_plan* plan, int kind);

/* per-kernel-launch view of the same numbers: one group = one kernel launch of the plan */
typedef struct {
  char     name[48];        /* e.g. "lev_wave<ALIGN,R=4>", "align_traceback", "lcf" */
  int32_t  kind;            /* enum pgpu_dp_kind */
  int32_t  pad;
  uint64_t jobs, cells, algo_bytes;
  double   ms;              /* HIP-event duration of the last launch */
  double   t0_ms;           /* its start on the device's time line: milliseconds since an event the library recorded
                               when the first context of the process came up -- the same line for every context on
                               the device, so the launches of several contexts can be merged into the time the device
                               was busy (bench.py: kernel_busy_union_ms); -1 when timing is off */
} pgpu_group_info;
int pgpu_dp_plan_n_groups(const pgpu_dp_plan* plan);
int pgpu_dp_plan_group_info(const pgpu_dp_plan* plan, int i, pgpu_group_info* out);

/* one-shot convenience: create + launch + sync + fetch + destroy */
int pgpu_dp_batch(pgpu_ctx* ctx, const pgpu_index* idx,
                  const pgpu_dp_job* jobs, size_t n_jobs, const char* arena, size_t arena_len,
                  pgpu_dp_result* results, char* strings, size_t strings_cap,
                  size_t* strings_used);

#ifdef __cplusplus
}
#endif
#endif
