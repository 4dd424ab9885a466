// The small stage for the queries the narrow kernel refuses for the prefix window alone.  Semantics:
// include/pintron_gpu.h (pgpu_index_small_chains_wide).
//
//   small_wide_kernel  the body of small_kernel (pgpu_small_body.h) at 16 rows of step 1's BORDERS body per lane: an allelen
//                      of up to PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW = 1024, every other cap as it is.  It runs behind
//                      small_kernel over the same arrays, on the same stream; one wave per workgroup, striding alike.  A wave
//                      takes only the queries with refused == 2, answers them from the input again, all steps, and
//                      overwrites the result, the list and the step bytes; a query that then meets another cap is refused
//                      with that cap's code.  Every other query is not touched, so the two kernels together equal
//                      small_kernel wherever that one answers, and the common case keeps its occupancy.
//                      LDS of a wave: the list (128 x 16), the four row-minimum arrays of the BORDERS mode (4 x 1025 words),
//                      the job's result (48), the step bytes (128) and the prefix piece (64): 18 688 bytes, nothing in HBM
//                      beside the call's block.
#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_lcf.h"
#include "pgpu_classify.h"
#include "pgpu_clean_body.h"
#include "pgpu_small_body.h"
#include "pgpu_stage_launch.h"

namespace {

static_assert(PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW == 16 * 64, "lev_wave_body<16, BORDERS>: sixteen rows of the pattern per lane");

__global__ __launch_bounds__(64)
void small_wide_kernel(const LcfIndexView ix, const ClassView cv, const uint8_t* __restrict__ ests,
                       const pgpu_factor* __restrict__ exons, const pgpu_small_query* __restrict__ queries, uint32_t n_queries,
                       const int min_intron_length, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps,
                       pgpu_small_result* __restrict__ out) {
  small_stage::small_body<16, true>(ix, cv, ests, exons, queries, n_queries, min_intron_length, out_exons, out_steps, out);
}

}  // namespace

void pgpu_small_wide_launch(const LcfIndexView& ix, const ClassView& cv, const uint8_t* ests, const pgpu_factor* exons,
                            const pgpu_small_query* q, uint32_t n, int min_intron_length, size_t waves, pgpu_factor* out_exons,
                            uint8_t* out_steps, pgpu_small_result* out, hipStream_t st) {
  pgpu_small_launch(ix, cv, ests, exons, q, n, min_intron_length, waves, out_exons, out_steps, out, st);
  hipLaunchKernelGGL(small_wide_kernel, dim3((unsigned)waves), dim3(64), 0, st, ix, cv, ests, exons, q, n, min_intron_length,
                     out_exons, out_steps, out);
}
