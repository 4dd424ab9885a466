// The chained stage kernels (clean_kernel, gaps_kernel, chain_kernel, tail_kernel, small_kernel) as plain launches over device pointers,
// for a caller that has the ESTs, the exons and the queries in HBM already: the factorization driver of pgpu_fact.hip (clean,
// gaps, refine) and the final driver of pgpu_final.hip behind it (tail, small).  Each of pgpu_clean.hip, pgpu_gaps.hip,
// pgpu_chain.hip, pgpu_tail.hip and pgpu_small.hip launches its
// kernel through the function below from its public entry too, so there is one launch per kernel.  Beside them the one rule of a public entry that the driver has to repeat on
// the device: what an end exon of a clean query asks of the per-wave workspace (clean_query_need), __host__ __device__ so
// that the entry's validator and the driver's hand-off kernel run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_index.h"

struct ClassView;          // pgpu_classify.h

// direction bytes of one end-exon alignment, as the plan builder sizes them: lev_wave<ALIGN> [step][64 lanes] of 1 B,
// align_band [row / 16][64 lanes] of 4 B
__host__ __device__ inline size_t dirs_wave(uint32_t lb) { return ((size_t)lb + 64) * 64; }
__host__ __device__ inline size_t dirs_band(uint32_t la) { return ((size_t)(la >> 4) + 1) * 256; }
__host__ __device__ inline size_t rows_bytes(uint32_t la, uint32_t lb) { return (2 * ((size_t)la + lb + 1) + 15) & ~(size_t)15; }

// the smallest workspace a clean call asks for (no end exon to align at all)
constexpr uint32_t CLEAN_WS_DIRS_MIN = 256, CLEAN_WS_ROWS_MIN = 16;

// what step 1 of the cleaning says of a query: the coordinate rules that follow hold for the queries that pass it
__host__ __device__ inline bool clean_passes_step1(const pgpu_factor* ex, uint32_t ne, uint32_t est_len) {
  if (ne == 1 && (ex[0].EST_start < 0 || (uint32_t)ex[0].EST_start >= est_len)) return false;
  int pe = -1, pg = -1;
  for (uint32_t k = 0; k < ne; ++k) {
    const pgpu_factor f = ex[k];
    if (f.EST_start > f.EST_end || f.GEN_start > f.GEN_end || f.EST_start < pe || f.GEN_start < pg) return false;
    pe = f.EST_end; pg = f.GEN_end;
  }
  return true;
}

// A clean query's own rules: an EST of at least one byte, and for what passes step 1 the my_asserts of
// src/est-factorizations.c:2140-2141 and :2199-2200 on its end exons (false: the query is refused) -- which, in the same
// pass, say what the two end-exon alignments need of a wave's workspace: ws_dirs and ws_rows are raised to it.  The
// coordinates lie inside [-1, length] already (factor_ok).
__host__ __device__ inline bool clean_query_need(const pgpu_factor* ex, uint32_t ne, uint32_t est_len, size_t glen, size_t& ws_dirs,
                                                 size_t& ws_rows) {
  if (est_len == 0) return false;
  if (!clean_passes_step1(ex, ne, est_len)) return true;
  const pgpu_factor head = ex[0], tail = ex[ne - 1];
  if (head.EST_start < 0 || head.GEN_start < 0 || (uint32_t)tail.EST_end >= est_len || (size_t)tail.GEN_end >= glen) return false;
  if (ne > PGPU_CLEAN_MAX_EXONS) return true;                                           // refused on the device
  for (int end = 0; end < 2; ++end) {
    const pgpu_factor f = end ? tail : head;
    const uint32_t la = (uint32_t)(f.EST_end - f.EST_start + 1), lb = (uint32_t)(f.GEN_end - f.GEN_start + 1);
    if (la > PGPU_CLEAN_MAX_END_EXON || lb > PGPU_CLEAN_MAX_END_EXON) continue;      // refused on the device
    const size_t d = la <= 64u ? dirs_wave(lb) : dirs_band(la);
    if (d > ws_dirs) ws_dirs = d;
    // (a single exon is aligned again as the head step trimmed it: to 64 EST bytes or fewer, lev_wave<ALIGN> takes it)
    if (ne == 1 && la > 64u && dirs_wave(lb) > ws_dirs) ws_dirs = dirs_wave(lb);
    if (rows_bytes(la, lb) > ws_rows) ws_rows = rows_bytes(la, lb);
  }
  return true;
}

// pgpu_clean.hip.  The grid of a clean call of n queries whose workspace was sized to (ws_dirs, ws_rows): `waves`
// workgroups of one wave, each with `ws_wave` bytes of the workspace (chained_waves, then the budget rule on the
// workspaces together).  The launch: `ws` holds waves * ws_wave bytes, `undersized` is a word the caller has set to 0.
hipError_t pgpu_clean_grid(size_t n, size_t ws_dirs, size_t ws_rows, size_t& waves, size_t& ws_wave);
void pgpu_clean_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_clean_query* q,
                       uint32_t n, uint8_t* ws, size_t ws_dirs, size_t ws_rows, size_t waves, pgpu_factor* out_exons,
                       uint8_t* out_marks, pgpu_clean_result* out, uint32_t* undersized, hipStream_t st);
// pgpu_gaps.hip: no workspace
void pgpu_gaps_launch(const uint8_t* T, const uint8_t* ests, const pgpu_factor* exons, const pgpu_gaps_query* q, uint32_t n,
                      size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_gaps_result* out, hipStream_t st);
// pgpu_chain.hip: `ws` holds waves * pgpu_chain_ws_wave() bytes
size_t pgpu_chain_ws_wave(void);
void pgpu_chain_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_chain_query* q,
                       uint32_t n, uint8_t* ws, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_chain_result* out,
                       hipStream_t st);
// pgpu_tail.hip: no workspace; tlen is the length of the resident sequence T
void pgpu_tail_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_tail_query* q,
                      uint32_t n, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out, hipStream_t st);
// pgpu_small.hip: no workspace; the views of the resident index (pgpu_index_lcf_view) and of its classification tables
// (pgpu_class_view_get); out_exons and out_steps hold two entries per exon of `exons`
void pgpu_small_launch(const LcfIndexView& ix, const ClassView& cv, const uint8_t* ests, const pgpu_factor* exons,
                       const pgpu_small_query* q, uint32_t n, int min_intron_length, size_t waves, pgpu_factor* out_exons,
                       uint8_t* out_steps, pgpu_small_result* out, hipStream_t st);
// pgpu_tail_wide.hip, pgpu_small_wide.hip: the narrow launch above, then the wide kernel over the same arrays on the same
// stream for the queries the narrow one refused for a window (tail: PGPU_ERANGE; small: refused == 2); the same `waves`
void pgpu_tail_wide_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_tail_query* q,
                           uint32_t n, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out, hipStream_t st);
void pgpu_small_wide_launch(const LcfIndexView& ix, const ClassView& cv, const uint8_t* ests, const pgpu_factor* exons,
                            const pgpu_small_query* q, uint32_t n, int min_intron_length, size_t waves, pgpu_factor* out_exons,
                            uint8_t* out_steps, pgpu_small_result* out, hipStream_t st);
