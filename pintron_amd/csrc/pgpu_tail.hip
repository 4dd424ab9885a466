// What est-fact does to a factorization directly behind the refinement loop, chained, on the resident index.  Semantics:
// include/pintron_gpu.h (pgpu_index_tail_chains): one query is one factorization, and the answer is what
// correct_composition_tail, detect_polyA_signal (src/detect-polya.c:42-166), remove_invalid_factorizations,
// recover_lost_prefixes_and_suffixes and remove_false_small_exons (src/factorization-refinement.c:120-165, :959-1266) make of it.
//
// The kernel's body is tail_body<4, false> of pgpu_tail_body.h, which tail_wide_kernel (pgpu_tail_wide.hip) shares at 16 rows
// per lane; pgpu_index_tail_chains_wide below queues that kernel behind this one.
//
//   tail_kernel     one wave per query (a workgroup is one wave); a wave that has finished a query takes the next one of
//                   its stride.  The exons sit in the wave's LDS, one lane loads one.  Step 1 compares 64 bytes per ballot.
//                   Steps 2 and 3 and the list edits of steps 4 and 5 are wave-uniform work on scalars.  The dynamic
//                   programs are the bodies of pgpu_wave_dp.h, unchanged, each at ONE call site and at the smallest
//                   rows-per-lane that holds its cap: lev_wave_body<4, AFFIX> (256 rows) for the lost prefix and the lost
//                   suffix, lev_wave_body<2, ED> (the shorter string on the rows: at most 100) for the three edit distances
//                   of an analysis, lev_wave_body<2, BORDERS> (128 rows) for its border refinement.  The prefix windows are
//                   read backwards from the exon: the wave writes the two reversed windows into LDS and hands the AFFIX body
//                   pointers to them.  A question the host code does not ask (equal first bytes, equal strings, an exon that
//                   is not analysed) runs no DP here either.  Everything that decides is uniform over the wave.
//                   LDS of a wave: the exons (64 x 16), the four row-minimum arrays of the BORDERS mode (4 x 129 words), the
//                   job's result (48), the step bytes (64) and the two reversed windows (256 + 304): 3 760 bytes, nothing
//                   in HBM beside the call's block.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_tail_body.h"
#include "pgpu_tail.h"
#include "pgpu_stage_launch.h"

namespace {

static_assert(PGPU_TAIL_MAX_AFFIX == 4 * 64, "lev_wave_body<4, AFFIX>: four rows of the EST window per lane");

__global__ __launch_bounds__(64)
void tail_kernel(const uint8_t* __restrict__ T, const uint32_t gl, const uint8_t* __restrict__ ests,
                 const pgpu_factor* __restrict__ exons, const pgpu_tail_query* __restrict__ queries, uint32_t n_queries,
                 pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps, pgpu_tail_result* __restrict__ out) {
  tail_stage::tail_body<4, false>(T, gl, ests, exons, queries, n_queries, out_exons, out_steps, out);
}

thread_local double t_tail_ms = 0.0;

}  // namespace

void pgpu_tail_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_tail_query* q,
                      uint32_t n, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out, hipStream_t st) {
  hipLaunchKernelGGL(tail_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, tlen, ests, exons, q, n, out_exons, out_steps, out);
}

extern "C" double pgpu_index_tail_chains_kernel_ms(void) { return t_tail_ms; }

// the entry in its two forms: `wide` queues tail_wide_kernel behind tail_kernel, inside the one event pair
static int tail_chains_call(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_factor* exons,
                            size_t n_exons_total, const pgpu_tail_query* q, size_t n, pgpu_factor* out_exons, uint8_t* out_steps,
                            pgpu_tail_result* out, const bool wide) {
  t_tail_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_tail_query) == 32 && sizeof(pgpu_tail_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, "queries", named);
  if (begun != CHAINED_GO) return begun;
  const size_t glen = pgpu_index_length(idx);
  const auto own = [=](const pgpu_tail_query& x, const pgpu_factor* ex) { return tail_query_ok(x, ex, ests_len, glen); };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, glen, named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad tail query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two "
                                           "queries share, or a coordinate that is no byte of what it indexes)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "tail chains");
  size_t waves = 0, cus = 0;
  TRY_HIP(chained_waves(n, waves, cus));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 0, 0);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(call.record(0));
  (wide ? pgpu_tail_wide_launch : pgpu_tail_launch)(pgpu_index_genomic(idx), (uint32_t)glen, call.d, (const pgpu_factor*)(call.d + L.exons),
      (const pgpu_tail_query*)(call.d + L.queries), (uint32_t)n, waves, (pgpu_factor*)(call.d + L.out_exons),
      call.d + L.out_bytes, (pgpu_tail_result*)(call.d + L.results), call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_steps, out));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_tail_ms);
  return PGPU_OK;
}

extern "C" int pgpu_index_tail_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                      const pgpu_factor* exons, size_t n_exons_total, const pgpu_tail_query* q, size_t n,
                                      pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out) {
  return tail_chains_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, false);
}

extern "C" int pgpu_index_tail_chains_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                           const pgpu_factor* exons, size_t n_exons_total, const pgpu_tail_query* q, size_t n,
                                           pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out) {
  return tail_chains_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, true);
}
