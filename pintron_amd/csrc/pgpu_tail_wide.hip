// The tail stage for the queries the narrow kernel refuses for a lost window alone.  Semantics: include/pintron_gpu.h
// (pgpu_index_tail_chains_wide).
//
//   tail_wide_kernel  the body of tail_kernel (pgpu_tail_body.h) at 16 rows of the AFFIX body per lane: a lost prefix or
//                     suffix of up to PGPU_TAIL_WIDE_MAX_AFFIX = 1024 EST bytes, every other cap as it is.  It runs behind
//                     tail_kernel over the same arrays, on the same stream; one wave per workgroup, striding alike.  A wave
//                     takes only the queries whose result is PGPU_ERANGE, answers them from the input again, all steps, and
//                     overwrites the result, the exons and the step bytes; a query that meets another cap is refused again:
//                     its result is written once more, the same PGPU_ERANGE bytes, its exons and step bytes are not.
//                     Every other query is not touched, so the two kernels together equal tail_kernel wherever that one
//                     answers, and the common case keeps its occupancy.
//                     LDS of a wave: the exons (64 x 16), the four row-minimum arrays of the BORDERS mode (4 x 129 words), the
//                     job's result (48), the step bytes (64) and the two reversed windows (1024 + 1200; (int)(1.17 * 1024) =
//                     1198 genomic bytes, rounded up to 16): 5 424 bytes, nothing in HBM beside the call's block (DESIGN.md
//                     section 5r).
#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_tail_body.h"
#include "pgpu_stage_launch.h"

namespace {

static_assert(PGPU_TAIL_WIDE_MAX_AFFIX == 16 * 64, "lev_wave_body<16, AFFIX>: sixteen rows of the EST window per lane");
static_assert((uint32_t)(1.17 * PGPU_TAIL_WIDE_MAX_AFFIX) == 1198 && tail_stage::tail_max_affix_gen<16>() == 1200, "the genomic window of a prefix");

__global__ __launch_bounds__(64)
void tail_wide_kernel(const uint8_t* __restrict__ T, const uint32_t gl, const uint8_t* __restrict__ ests,
                      const pgpu_factor* __restrict__ exons, const pgpu_tail_query* __restrict__ queries, uint32_t n_queries,
                      pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps, pgpu_tail_result* __restrict__ out) {
  tail_stage::tail_body<16, true>(T, gl, ests, exons, queries, n_queries, out_exons, out_steps, out);
}

}  // namespace

void pgpu_tail_wide_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_tail_query* q,
                           uint32_t n, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_tail_result* out, hipStream_t st) {
  pgpu_tail_launch(T, tlen, ests, exons, q, n, waves, out_exons, out_steps, out, st);
  hipLaunchKernelGGL(tail_wide_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, tlen, ests, exons, q, n, out_exons, out_steps, out);
}
