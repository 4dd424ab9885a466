// Intron borders from the gap alignment, on the resident index.  Semantics: include/pintron_gpu.h
// (pgpu_index_refine_introns); the decision is refine_intron's (src/refine-intron.c:47-265) as
// pintron_amd/host/ef_refine_intron.c:455-509 restates it, routine by routine.
//
//   refine_kernel   one wave per query.  The two rows are staged in LDS once.  Everything that decides is uniform
//                   over the wave; the lanes share the work that has a width: the strlen of the rows, the counts of
//                   non-gap columns, the two dinucleotide scans that do not skip gaps (64 columns per ballot), the
//                   staging of the operands and the edit distances (one anti-diagonal per step, its cells over the
//                   lanes, three diagonals in LDS).  Both cycles of a shift variant are found before any distance; the
//                   at most six distances of that variant follow; the next variant runs only when this one did not
//                   settle.  The two scans that skip gap columns and the Burset walk are short dependent chains and run
//                   as the host code has them.
#include <string.h>

#include "pgpu_query_call.h"
#include "pgpu_refine_body.h"

namespace {

__global__ __launch_bounds__(64)
void refine_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint8_t* __restrict__ ests, const uint8_t* __restrict__ rows,
                   const pgpu_refine_query* __restrict__ queries, pgpu_refine_result* __restrict__ out) {
  __shared__ RefineLds L;
  const int lane = (int)threadIdx.x;
  const pgpu_refine_query q = queries[blockIdx.x];
  pgpu_refine_result r;
  r.status = PGPU_OK; r.refined = 0; r.path = 0; r.pad = 0; r.donor = q.donor; r.acceptor = q.acceptor;
  if (q.dim > (uint32_t)MAX_DIM) {
    r.status = PGPU_ERANGE;
  } else {
    const int dim = (int)q.dim;
    for (int k = lane; k < 2 * dim; k += 64) L.rows[k] = rows[q.rows_off + (uint64_t)k];
    __syncthreads();
    refine_decide(L, L.rows, L.rows + dim, dim, q, T, n, ests, lane, r);
  }
  if (lane == 0) out[blockIdx.x] = r;
}

thread_local double t_refine_ms = 0.0;

}  // namespace

extern "C" double pgpu_index_refine_introns_kernel_ms(void) { return t_refine_ms; }

extern "C" int pgpu_index_refine_introns(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                         const char* rows, size_t rows_len,
                                         const pgpu_refine_query* q, size_t n, pgpu_refine_result* out) {
  t_refine_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_refine_query) == 96 && sizeof(pgpu_refine_result) == 48 && sizeof(pgpu_factor) == 16, "ABI layout");
  if (!ctx || !idx || (n && (!q || !out)) || (ests_len && !ests) || (rows_len && !rows)) return PGPU_EINVAL;
  if (n > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 queries in one call");
  const size_t glen = pgpu_index_length(idx);
  for (size_t i = 0; i < n; ++i) {
    const pgpu_refine_query& x = q[i];
    bool ok = x.est_off <= ests_len && x.est_len <= ests_len - x.est_off && x.dim != 0 && x.rows_off <= rows_len &&
              2ull * x.dim <= rows_len - x.rows_off && (x.flags & ~PGPU_REFINE_FIRST_INTRON) == 0 &&
              x.donor.EST_end < x.acceptor.EST_start && x.donor.GEN_end < x.acceptor.GEN_start;
    ok = ok && factor_ok(x.donor, x.est_len, glen) && factor_ok(x.acceptor, x.est_len, glen) &&
         suffpref_ok(x.suffpref_length_on_est, x.suffpref_length_for_intron, x.suffpref_length_on_gen);
    for (int32_t v : { x.factor_cut, x.intron_start, x.intron_end, x.intron_start_on_align, x.intron_end_on_align })
      ok = ok && v >= 0 && (uint32_t)v <= x.dim;
    if (!ok)
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad refine query (an offset past its buffer, an unknown flag, dim == 0, a donor that is "
                                             "not in front of the acceptor, or a coordinate outside what it indexes)");
  }
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "refine_introns");
  const hipStream_t st = call.st;
  const size_t o_rows = up256(ests_len + 64), o_q = o_rows + up256(rows_len + 64), o_r = o_q + up256(n * sizeof(pgpu_refine_query)),
               total = o_r + up256(n * sizeof(pgpu_refine_result));
  TRY_HIP(hipMalloc((void**)&call.d, total));
  TRY_HIP(call.timing_events(1));
  if (ests_len) TRY_HIP(hipMemcpyAsync(call.d, ests, ests_len, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(call.d + o_rows, rows, rows_len, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(call.d + o_q, q, n * sizeof(pgpu_refine_query), hipMemcpyHostToDevice, st));
  TRY_HIP(call.record(0));
  hipLaunchKernelGGL(refine_kernel, dim3((unsigned)n), dim3(64), 0, st, pgpu_index_genomic(idx), (uint32_t)glen, call.d, call.d + o_rows,
                     (const pgpu_refine_query*)(call.d + o_q), (pgpu_refine_result*)(call.d + o_r));
  TRY_HIP(call.record(1));
  TRY_HIP(hipMemcpyAsync(out, call.d + o_r, n * sizeof(pgpu_refine_result), hipMemcpyDeviceToHost, st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_refine_ms);
  return PGPU_OK;
}
