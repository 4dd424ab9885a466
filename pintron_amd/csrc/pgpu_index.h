// Internal view of the genomic index (pgpu_index.hip) and of the context, for the library's other files.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <hip/hip_runtime.h>
#include "../../include/pintron_gpu.h"

const uint8_t* pgpu_index_genomic(const pgpu_index* idx);   // device pointer
size_t pgpu_index_length(const pgpu_index* idx);

// width of the k-mer interval table (klo / khi): 4^KTAB entries each, upper-case ACGT k-mers only; an absent
// k-mer has klo == khi
constexpr uint32_t KTAB = 8;
constexpr uint32_t KTAB_ENTRIES = 1u << (2 * KTAB);
__device__ __forceinline__ int kmer_base(uint32_t c) {
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}
// 2-bit code of s[0..KTAB), or -1 when a character is not A/C/G/T (`avail` readable characters)
__device__ __forceinline__ int kmer_code(const uint8_t* __restrict__ s, uint32_t avail) {
  if (avail < KTAB) return -1;
  int code = 0;
#pragma unroll
  for (uint32_t x = 0; x < KTAB; ++x) {
    const int b = kmer_base(s[x]);
    if (b < 0) return -1;
    code = (code << 2) | b;
  }
  return code;
}

// What the suffix-array form of find_longest_common_factor_dp needs (pgpu_dp_kernels.hip: lcfsa_wave_body):
//   focc   first occurrence of every upper-case ACGT l-mer, l = 1..8 (table l at offset (4^l - 4) / 3;
//          0xFFFFFFFF: the l-mer does not occur)
//   rmq    sparse table of range minima over the suffix array: level j >= 1 at (j-1) * n holds
//          min(sa[k .. k + 2^j)) for k + 2^j <= n; level 0 is the suffix array itself
//   klo, khi  the k-mer interval table above; T, sa, n: the sequence (n bytes), its suffix array
//   first_bad  position of the first character of the sequence that is not an upper-case A, C, G or T
//          (n when there is none): prefixes up to there can be searched with exact matching alone
struct LcfIndexView {
  const uint8_t* T; const uint32_t* sa; const uint32_t* klo; const uint32_t* khi; const uint32_t* focc; const uint32_t* rmq;
  uint32_t n, levels, first_bad;
};
LcfIndexView pgpu_index_lcf_view(const pgpu_index* idx);
// the small stage's view (pgpu_index_small_chains, pgpu_final_job): without the derived tables every prefix question is refused = 3
inline LcfIndexView pgpu_index_small_view(const pgpu_index* idx) {
  LcfIndexView ix = pgpu_index_lcf_view(idx);
  if (!ix.focc || !ix.rmq) ix.first_bad = 0;
  return ix;
}
constexpr uint32_t LCF_FOCC_ENTRIES = 87380;      // 4 + 16 + ... + 4^8

// What the pairing kernels need (pgpu_pairing_plan.hip): the sequence T (n bytes), its suffix array and LCP array
// (n + 1 entries), the k-mer interval table, the alphabet keys of preprocess_text (256 entries; sigma = number of
// distinct characters), and the sequence at 2 bits per base with its flag bits (pack_sequence).
struct PairIndexView {
  const uint8_t* T; uint32_t n; const uint32_t* sa; const uint32_t* lcp; const uint32_t* klo; const uint32_t* khi;
  const uint8_t* key; uint32_t sigma; const uint32_t* code; const uint32_t* bad;
};
PairIndexView pgpu_index_pair_view(const pgpu_index* idx);
// src[0..n) (device) -> code (2 * ceil(n / 32) words, + 4 of slack the windows may read) and flag words (ceil(n / 32) + 4):
// 2 bits per base, and one flag bit per base that is not an upper-case A, C, G or T
hipError_t pack_sequence(const uint8_t* src, size_t n, uint32_t* code, uint32_t* bad, hipStream_t st);

// Tables that are derived from the sequence on first use and then belong to the index (the classification tables
// of pgpu_classify.hip): whoever needs them takes `mu`, builds when `tables` is still null, and leaves `release`
// for pgpu_index_destroy.  An index is shared by many contexts, so two of them may ask at the same time.
struct pgpu_index_lazy { std::mutex mu; void* tables = nullptr; void (*release)(void*) = nullptr; };
pgpu_index_lazy* pgpu_index_lazy_slot(const pgpu_index* idx);

// context helpers implemented in pgpu_api.hip
hipStream_t pgpu_ctx_stream(pgpu_ctx* ctx);
// makes the context's device current on the calling thread (HIP's current device is per thread:
// a fresh prefetch or service thread starts on device 0)
int pgpu_ctx_bind(pgpu_ctx* ctx);
// waits for everything queued on the context's stream WITHOUT spinning: HIP's own stream synchronisation
// busy-waits, and the thread that drives the pairing / MEG prefetch would burn a core of the host's CPU quota
// for the tens of milliseconds per step its kernels run (PGPU_WAIT: the nap in microseconds, as for DP plans)
hipError_t pgpu_ctx_wait(pgpu_ctx* ctx);
int pgpu_ctx_fail(pgpu_ctx* ctx, int code, const char* msg);
// the context's two pools of device buffers (BufPool, pgpu_api.hip): DP plans keep one block in pool 0; the slots of
// pool 1 are named after what a pairing plan keeps in them, and their number is the size of every pool
constexpr int PLAN_POOL = 1;
enum PlanSlot : int {
  SLOT_PATS, SLOT_PAT_OFF,
  SLOT_LO, SLOT_HI, SLOT_A, SLOT_THR, SLOT_CNT, SLOT_CNT_A, SLOT_CNT_B, SLOT_CAND_OFF, SLOT_OUT_OFF, SLOT_OUT_FIRST, SLOT_TMP,
  SLOT_CAND, SLOT_KEEP, SLOT_OUT,
  SLOT_MEG_SCRATCH, SLOT_MEG_INFO, SLOT_MEG_BYTES, SLOT_MEG_OFF, SLOT_MEG_OUT,
  SLOT_PCODE, SLOT_PBAD,
  SLOT_CAND_RES, SLOT_CAND_CNT, SLOT_CAND_FIRST, SLOT_CAND_EXONS,
  SLOT_FACT, SLOT_FACT_WS,
  SLOT_ORIG_OFF, SLOT_FINAL,
  SLOT_UNITS,
  SLOT_TEXTS, SLOT_TEXT_BLOBS,
  SLOT_SIDES, SLOT_SIDE_BLOBS,
  SLOT_ENUM, SLOT_ENUM_OUT,
  SLOT_FLIST, SLOT_FLIST_WS,
  PLAN_SLOTS
};
bool pgpu_ctx_pool_acquire(pgpu_ctx* ctx, int pool);
void pgpu_ctx_pool_release(pgpu_ctx* ctx, int pool);
void* pgpu_ctx_pool_get(pgpu_ctx* ctx, int pool, int slot, size_t bytes);
bool pgpu_ctx_pool_share(pgpu_ctx* ctx, int pool);
void pgpu_ctx_pool_unshare(pgpu_ctx* ctx, int pool, const void* who);
void pgpu_ctx_pool_set_owner(pgpu_ctx* ctx, int pool, const void* who);
const void* pgpu_ctx_pool_owner(const pgpu_ctx* ctx, int pool);
bool pgpu_ctx_timing(const pgpu_ctx* ctx);
// what an entry returns for a HIP error
inline int pgpu_code_of(hipError_t e) { return e == hipErrorOutOfMemory ? PGPU_ENOMEM : PGPU_EDEVICE; }
// a profiler range (pgpu_range_push / pgpu_range_pop) that ends with its scope
struct ProfRange {
  explicit ProfRange(const char* name) { pgpu_range_push(name); }
  ~ProfRange() { pgpu_range_pop(); }
  ProfRange(const ProfRange&) = delete;
  ProfRange& operator=(const ProfRange&) = delete;
};

// pgpu_meg.hip: hand-written exclusive prefix sums and the per-pattern MEG kernels
size_t pgpu_scan_tmp_bytes(size_t n);
void pgpu_exclusive_scan_u32(const uint32_t* in, unsigned long long* out, size_t n, void* tmp, hipStream_t st);
size_t pgpu_meg_scratch_bytes(size_t n_pat);
void pgpu_meg_launch_build(const pgpu_pairing* pairs, const unsigned long long* pair_first, const unsigned long long* pat_off,
                           uint32_t n_pat, const pgpu_meg_params* prm, void* scratch, void* info, uint32_t* rec_bytes,
                           hipStream_t st);
void pgpu_meg_launch_emit(uint32_t n_pat, const void* scratch, const void* info, const unsigned long long* rec_off,
                          uint8_t* out, hipStream_t st);
// pgpu_cand.hip: the candidate factorization of every record of a batch of MEG records, in two launches around an exclusive
// scan of `counts` (n + 1 entries, the last one 0): the count pass fills res and counts, the write pass first_exon and exons
void pgpu_cand_launch_count(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                            const pgpu_cand_params* prm, pgpu_cand_result* res, uint32_t* counts, hipStream_t st);
void pgpu_cand_launch_write(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                            const pgpu_cand_params* prm, pgpu_cand_result* res, const unsigned long long* first_exon,
                            pgpu_factor* exons, hipStream_t st);
// pgpu_enum.hip: every candidate of every record of a batch of MEG records, in two launches around two exclusive scans (of
// cnt_c and cnt_e, n + 1 entries each, the last one 0): the count pass fills res and the counts, the write pass
// first_candidate, the candidate table and the exons.  The error is that of asking the device for its grid.
hipError_t pgpu_enum_launch_count(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                                  const pgpu_cand_params* prm, pgpu_enum_result* res, uint32_t* cnt_c, uint32_t* cnt_e, hipStream_t st);
hipError_t pgpu_enum_launch_write(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                                  const pgpu_cand_params* prm, pgpu_enum_result* res, const unsigned long long* first_c,
                                  const unsigned long long* first_e, pgpu_enum_candidate* cands, pgpu_factor* exons, hipStream_t st);
// pgpu_fact.hip: the candidates of n ESTs through clean, gaps and refine, all on the device.  The caller fills everything but
// the two results; `block` holds fact_layout(n, n_exons_total, pgpu_scan_tmp_bytes(n + 1)).total bytes (pgpu_fact.h), where
// the outcomes (res), the compact exons and their step bytes are found afterwards.  The candidates are either queries
// (fq) or a plan's pattern offsets and candidate results (pat_off, cand; fq null); cand_exons may be the block's ex_in
// itself.  ws_alloc is asked once, for the workspace of clean and refine, after the call's one host wait; the drive ends with
// a second wait, so `total` (exons of the answer) and `undersized` (clean's flag: the call failed) are set on return.
struct pgpu_fact_job {
  const uint8_t* T; uint32_t tlen;
  const uint8_t* ests;
  const pgpu_fact_query* fq;
  const unsigned long long* pat_off; const pgpu_cand_result* cand;
  const pgpu_factor* cand_exons;
  uint32_t n, n_exons_total;
  uint8_t* block;
  void* (*ws_alloc)(void* user, size_t bytes); void* ws_user;
  hipEvent_t ev[8];            // the caller's (QueryCall, plan); null without timing: 0-1 the whole drive, 2-3 clean, 4-5 gaps, 6-7 chain
  unsigned long long total; uint32_t undersized;
};
hipError_t pgpu_fact_drive(pgpu_ctx* ctx, pgpu_fact_job& job, const pgpu_fact_params& prm);
// what an entry answers to a job that comes back `undersized`; `what`: the entry's noun
inline int pgpu_clean_undersized(pgpu_ctx* ctx, const char* what) {
  char msg[128];
  snprintf(msg, sizeof msg, "%s: the workspace of a wave was sized too small for an end-exon alignment", what);
  return pgpu_ctx_fail(ctx, PGPU_EDEVICE, msg);
}
// pgpu_flists.hip: the candidate lists of n ESTs (`cands`: n_cands entries, `cand_exons`: n_exons_total, both in HBM) through
// clean, the selection (add_if_not_exists, FILTER 1, FILTER 3), gaps and refine, all on the device.  `block` holds
// flist_layout(n, n_cands, n_exons_total, pgpu_scan_tmp_bytes(n + 1)).total bytes (pgpu_flists.h), where the outcomes (res), the
// factorizations (facts), the compact exons and their step bytes are found afterwards.  The ESTs are either queries (q) or a
// plan's pattern offsets and enumeration results (pat_off, enum_res; q null); cand_exons may be the block's ex_in itself.
// ws_alloc, the two waits and `undersized` as in pgpu_fact_job.
struct pgpu_flist_job {
  const uint8_t* T; uint32_t tlen;
  const uint8_t* ests;
  const pgpu_flist_query* q;
  const unsigned long long* pat_off; const pgpu_enum_result* enum_res;
  const pgpu_enum_candidate* cands; const pgpu_factor* cand_exons;
  uint32_t n, n_cands, n_exons_total;
  uint8_t* block;
  void* (*ws_alloc)(void* user, size_t bytes); void* ws_user;
  hipEvent_t ev[10];           // null without timing: 0-1 the whole drive, 2-3 clean, 4-5 select, 6-7 gaps, 8-9 chain
  unsigned long long total_facts, total_exons; uint32_t undersized;
  // Null in every call of the library.  pgpu_flist_handoffs_probe sets it: host arrays in the layout of the block's gr
  // (n_cands), ex_gaps and gsteps (n_exons_total + n_cands each) that are copied in where gaps_kernel would have written
  // them, and the kernel is not launched -- the hand-off kernels behind it then run over results no input brings through
  // gaps_kernel (two kept exons out of order)
  struct Given { const pgpu_gaps_result* results; const pgpu_factor* exons; const uint8_t* steps; };
  const Given* given_gaps;
};
hipError_t pgpu_flist_drive(pgpu_ctx* ctx, pgpu_flist_job& job, const pgpu_flist_params& prm);
// pgpu_final.hip: the answer of pgpu_fact_drive, where it lies (`fact_block`, the block of a job of the same n and
// n_exons_total, read only), through the tail and the small stage.  The ESTs are either the queries of the index form (fq) or
// a plan's pattern offsets and its table of original offsets (pat_off, orig_off; fq null); `ests_len` bytes lie behind
// `ests`, originals included.  `block` holds final_layout(n, n_exons_total, pgpu_scan_tmp_bytes(n + 1)).total bytes
// (pgpu_final.h), where the outcomes (res), the compact exons and their step bytes are found afterwards.  The one host wait
// of the drive is its last statement: `total` (exons of the answer) is set on return.
struct ClassView;          // pgpu_classify.h
struct pgpu_final_job {
  LcfIndexView ix; const ClassView* cv;
  const uint8_t* ests; size_t ests_len;
  const pgpu_final_query* fq;
  const unsigned long long* pat_off; const unsigned long long* orig_off;
  const uint8_t* fact_block;
  uint32_t n, n_exons_total;
  int min_intron_length;
  uint8_t* block;
  hipEvent_t ev[6];            // null without timing: 0-1 the whole drive, 2-3 tail_kernel, 4-5 small_kernel
  unsigned long long total;
  // the wide form: tail_wide_kernel and small_wide_kernel are queued behind the two stage kernels (pgpu_tail_wide_launch,
  // pgpu_small_wide_launch), inside the event pairs 2-3 and 4-5
  bool wide = false;
  // Null in every call of the library.  pgpu_final_handoffs_probe sets both: host arrays in the layout of the block's
  // tr / ex_tout / tsteps and sr / ex_sout / ssteps that are copied in where the stage kernel would have written them, and
  // the kernel is not launched -- the hand-off kernels then run over results no input brings through the stages.
  struct Given { const void* results; const pgpu_factor* exons; const uint8_t* steps; };
  const Given* given_tail = nullptr; const Given* given_small = nullptr;
};
hipError_t pgpu_final_drive(pgpu_ctx* ctx, pgpu_final_job& job);
// pgpu_unit.hip: the finals of the patterns (`res`, `exons`: n_exons_total entries, read only, where they lie) to one verdict
// per unit and the groups of the ALIGNED ones.  The empty-graph bit of a pattern is either a byte per pattern (`empty`, may
// be null: no graph is empty) or read from the header of its MEG record (`recs`, `rec_first`; `empty` is then not looked at).
// `n_done_exons`: the exons of the DONE results in all (the compact array of the final driver: n_exons_total itself).
// `block` holds unit_layout(n, n_done_exons, pgpu_scan_tmp_bytes(n + 1)).total bytes (pgpu_unit.h) with the n queries
// already at its `q`; the results (out) and the blob are found there afterwards.  The one host wait of the drive is its
// last statement: `total` (bytes of the blob) is set on return.
struct pgpu_unit_job {
  const pgpu_final_result* res; const pgpu_factor* exons; uint32_t n_exons_total; size_t n_done_exons;
  const uint8_t* empty;
  const uint8_t* recs; const unsigned long long* rec_first;
  pgpu_unit_params params;
  uint32_t n;
  uint8_t* block;
  hipEvent_t ev[2];            // null without timing: around count + scan + write
  unsigned long long total;
};
hipError_t pgpu_unit_drive(pgpu_ctx* ctx, pgpu_unit_job& job);
// pgpu_text.hip: the units and their groups (`units`, `blob`: read only, where they lie) to the two texts of every ALIGNED
// unit.  Sequence p is seqs[seq_at[p] ..) of seq_off[p + 1] - seq_off[p] bytes (the form without a plan: both are its
// seq_first; a plan: its table of original offsets and its pattern offsets).  Behind headers, sequences and genomic lie
// 16 readable bytes.  `block` holds text_layout(n, headers_len, pgpu_scan_tmp_bytes(n + 1)).total bytes (pgpu_text.h) with
// the headers and their offsets already in place.  pgpu_text_count runs the count pass and the two scans and ends with the
// stage's one host wait: the totals are set on return.  pgpu_text_write queues the write pass into two blobs of at
// least those sizes, and waits for nothing.
struct pgpu_text_job {
  const pgpu_unit_result* units; uint32_t n;
  const uint8_t* blob; unsigned long long blob_len;
  size_t headers_len;
  const uint8_t* seqs; const unsigned long long* seq_at; const unsigned long long* seq_off; uint32_t n_pat;
  const uint8_t* genomic; unsigned long long genomic_len;
  uint8_t* block;
  hipEvent_t ev[3];            // null without timing: 0-1 around count + scans + write, 2 in front of the write pass
  unsigned long long raw_total, pests_total;
};
hipError_t pgpu_text_count(pgpu_ctx* ctx, pgpu_text_job& job);
hipError_t pgpu_text_write(pgpu_ctx* ctx, const pgpu_text_job& job, uint8_t* raw, uint8_t* pests);
// the genomic sequence of pgpu_text_source_create: device pointer (16 readable bytes behind it), length, owner
struct pgpu_text_source { pgpu_ctx* owner; uint8_t* d; size_t len; };
// pgpu_side.hip: the queries and results of the unit stage (`q`, `units`: read only, where they lie) and the MEG records of
// the patterns (`recs`: recs_len bytes, record p at rec_first[p], n_pat + 1 offsets, every one a multiple of 4 and the base
// a multiple of 256) to the three side texts of every settled unit.  Headers (`hdr`, n + 1 offsets `hdr_first`) and
// sequences (as in pgpu_text_job) are read where they lie, with 16 readable bytes behind them.  `block` holds
// side_layout(n, pgpu_scan_tmp_bytes(n + 1)).total bytes (pgpu_side.h).  pgpu_side_count runs the count pass and the three
// scans and ends with the stage's one host wait: total[0 .. 3) are set on return.  pgpu_side_write queues the write pass
// into three blobs of at least those sizes, and waits for nothing.
struct pgpu_side_job {
  const pgpu_unit_query* q; const pgpu_unit_result* units; uint32_t n;
  const uint8_t* recs; unsigned long long recs_len; const unsigned long long* rec_first; uint32_t n_pat;
  const uint8_t* hdr; const unsigned long long* hdr_first;
  const uint8_t* seqs; const unsigned long long* seq_at; const unsigned long long* seq_off;
  uint8_t* block;
  hipEvent_t ev[3];            // null without timing: 0-1 around count + scans + write, 2 in front of the write pass
  unsigned long long total[3]; // megs, pmegs, edges
};
hipError_t pgpu_side_count(pgpu_ctx* ctx, pgpu_side_job& job);
hipError_t pgpu_side_write(pgpu_ctx* ctx, const pgpu_side_job& job, uint8_t* megs, uint8_t* pmegs, uint8_t* edges);
// PGPU_TRACE_ALLOC=1: every page-locked host allocation of the library on stderr (size, address, call site)
static inline void pgpu_trace_alloc(const char* what, const void* q, size_t bytes) {
  static int on = -1;
  if (on < 0) { const char* e = getenv("PGPU_TRACE_ALLOC"); on = (e && *e && *e != '0') ? 1 : 0; }
  if (on) fprintf(stderr, "* alloc %-18s %10.1f MB at %p\n", what, bytes / 1048576.0, q);
}

