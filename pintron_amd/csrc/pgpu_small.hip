// The last two routines of refine_EST_factorizations that concern one factorization alone, chained, on the resident index.
// Semantics: include/pintron_gpu.h (pgpu_index_small_chains): one query is one factorization as pgpu_index_tail_chains left
// it, and the answer is what search_for_new_small_exons (src/factorization-refinement.c:875-912, with
// search_small_exon_at_prefix :500-606 and search_small_exon :641-871) and clean_factorizations (:914-950) make of it.
//
// The kernel's body is small_body<4, false> of pgpu_small_body.h, which small_wide_kernel (pgpu_small_wide.hip) shares at 16
// rows per lane; pgpu_index_small_chains_wide below queues that kernel behind this one.
//
//   small_kernel    one wave per query (a workgroup is one wave); a wave that has finished a query takes the next one of
//                   its stride.  A lane keeps one exon of the input in registers; the list that grows is written to the
//                   wave's LDS from the left: the exon at hand (`cur`) stays in scalars until the pair behind it has been
//                   looked at, since an insertion moves its end.  Every question is a device routine that exists, at one
//                   call site each but the short edit distance (two): lcfsa_wave_key over the piece in LDS (once, or four
//                   times with the one N replaced), lev_wave_body<1, ED> (at most 23 rows), lev_wave_body<4, BORDERS> (256
//                   rows) for the prefix, lcf_small_wave_body (23 x 23), classify_intron, sexon_search, and for the last
//                   cleaning lev_wave_body<1, KBAND> (kband_band_sweep, or the whole matrix of a short exon), the best-run
//                   rule and external_exon_ok.  Everything that decides is uniform over the wave.
//                   LDS of a wave: the list (128 x 16), the four row-minimum arrays of the BORDERS mode (4 x 257 words), the
//                   job's result (48), the step bytes (128) and the prefix piece (64): 6 400 bytes, nothing in HBM beside
//                   the call's block.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_lcf.h"
#include "pgpu_classify.h"
#include "pgpu_clean_body.h"
#include "pgpu_small_body.h"
#include "pgpu_small.h"
#include "pgpu_stage_launch.h"

namespace {

static_assert(PGPU_SMALL_MAX_PREFIX_WINDOW == 4 * 64, "lev_wave_body<4, BORDERS>: four rows of the pattern per lane");

__global__ __launch_bounds__(64)
void small_kernel(const LcfIndexView ix, const ClassView cv, const uint8_t* __restrict__ ests,
                  const pgpu_factor* __restrict__ exons, const pgpu_small_query* __restrict__ queries, uint32_t n_queries,
                  const int min_intron_length, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps,
                  pgpu_small_result* __restrict__ out) {
  small_stage::small_body<4, false>(ix, cv, ests, exons, queries, n_queries, min_intron_length, out_exons, out_steps, out);
}

thread_local double t_small_ms = 0.0;

}  // namespace

void pgpu_small_launch(const LcfIndexView& ix, const ClassView& cv, const uint8_t* ests, const pgpu_factor* exons,
                       const pgpu_small_query* q, uint32_t n, int min_intron_length, size_t waves, pgpu_factor* out_exons,
                       uint8_t* out_steps, pgpu_small_result* out, hipStream_t st) {
  hipLaunchKernelGGL(small_kernel, dim3((unsigned)waves), dim3(64), 0, st, ix, cv, ests, exons, q, n, min_intron_length, out_exons,
                     out_steps, out);
}

extern "C" double pgpu_index_small_chains_kernel_ms(void) { return t_small_ms; }

// the entry in its two forms: `wide` queues small_wide_kernel behind small_kernel, inside the one event pair
static int small_chains_call(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_factor* exons,
                             size_t n_exons_total, const pgpu_small_query* q, size_t n, const pgpu_small_params* params,
                             pgpu_factor* out_exons, uint8_t* out_steps, pgpu_small_result* out, const bool wide) {
  t_small_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_small_query) == 32 && sizeof(pgpu_small_result) == 24 && sizeof(pgpu_small_params) == 8 &&
                sizeof(pgpu_factor) == 16, "ABI layout");
  if (!ctx || !idx || !params) return PGPU_EINVAL;
  // before chained_begin, whose empty call writes the outputs: a refused call leaves them untouched
  if (!small_params_ok(params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, SMALL_BAD_PARAMS);
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, "queries", named, 2);
  if (begun != CHAINED_GO) return begun;
  const size_t glen = pgpu_index_length(idx);
  const auto own = [=](const pgpu_small_query& x, const pgpu_factor* ex) { return small_query_ok(x, ex, ests_len, glen); };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, glen, named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad small query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two "
                                           "queries share, or a coordinate that is no byte of what it indexes)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  ClassView cv;
  const int rc = pgpu_class_view_get(ctx, idx, &cv);
  if (rc != PGPU_OK) return rc;
  QueryCall call(ctx, "small chains");
  size_t waves = 0, cus = 0;
  TRY_HIP(chained_waves(n, waves, cus));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 0, 0, 2);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(call.record(0));
  (wide ? pgpu_small_wide_launch : pgpu_small_launch)(pgpu_index_small_view(idx), cv, call.d, (const pgpu_factor*)(call.d + L.exons),
                    (const pgpu_small_query*)(call.d + L.queries), (uint32_t)n, params->min_intron_length, waves,
                    (pgpu_factor*)(call.d + L.out_exons), call.d + L.out_bytes, (pgpu_small_result*)(call.d + L.results), call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_steps, out));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_small_ms);
  return PGPU_OK;
}

extern "C" int pgpu_index_small_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                       const pgpu_factor* exons, size_t n_exons_total, const pgpu_small_query* q, size_t n,
                                       const pgpu_small_params* params, pgpu_factor* out_exons, uint8_t* out_steps,
                                       pgpu_small_result* out) {
  return small_chains_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, params, out_exons, out_steps, out, false);
}

extern "C" int pgpu_index_small_chains_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                            const pgpu_factor* exons, size_t n_exons_total, const pgpu_small_query* q, size_t n,
                                            const pgpu_small_params* params, pgpu_factor* out_exons, uint8_t* out_steps,
                                            pgpu_small_result* out) {
  return small_chains_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, params, out_exons, out_steps, out, true);
}
