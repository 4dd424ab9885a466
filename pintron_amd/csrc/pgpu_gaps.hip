// check_gap_errors of a factorization, chained, on the resident index.  Semantics: include/pintron_gpu.h
// (pgpu_index_gap_chains): one query is one factorization at FILTER 4 of get_EST_factorizations
// (src/est-factorizations.c:416-433, the routine at :1462-1545), and the answer is its verdict with the exons as the
// border loop and the merging loop left them.
//
//   gaps_kernel     one wave per query (a workgroup is one wave); a wave that has finished a query takes the next one of
//                   its stride.  The exons sit in the wave's LDS, one lane loads one.  The gaps are taken one after the
//                   other: the wave builds the PGPU_DP_BORDERS job of a gap in registers (a = the EST gap, b = the
//                   resident sequence behind the donor, p0 = 0, p1 = p2 = the gap's length, tail = 0) and runs
//                   lev_wave_body<1, BORDERS> of pgpu_wave_dp.h on it -- the code of that job in a plan, one row per
//                   lane -- then lane 0 moves the four ends that face the gap.  A gap of no EST byte runs no DP.  The
//                   merging loop is lane 0's walk over the list in LDS; the exons and their step bytes are written
//                   once, by their lanes.  Everything that decides is uniform over the wave.
//                   LDS of a wave: the exons (64 x 16), the four row-minimum arrays of the BORDERS mode (4 x 65 words),
//                   the job's result (48) and the step bytes (64): 2 176 bytes, nothing in HBM beside the call's
//                   block.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_gaps.h"
#include "pgpu_stage_launch.h"

namespace {

constexpr uint32_t MAX_EXONS = PGPU_GAPS_MAX_EXONS;
constexpr uint32_t MAX_EST_GAP = PGPU_GAPS_MAX_EST_GAP;
static_assert(MAX_EXONS == 64, "one lane per exon");
static_assert(MAX_EST_GAP == 64, "lev_wave_body<1, BORDERS>: one row of the pattern per lane");

struct GapsLds {
  pgpu_factor ex[MAX_EXONS];                  // the query's exons as the two loops leave them
  uint32_t rowmin[4 * (MAX_EST_GAP + 1)];     // pre, pre_pos, suf, suf_pos of the gap at hand
  DevResult res;                              // ... and its answer
  uint8_t steps[MAX_EXONS];
};

__global__ __launch_bounds__(64)
void gaps_kernel(const uint8_t* __restrict__ T, const uint8_t* __restrict__ ests, const pgpu_factor* __restrict__ exons,
                 const pgpu_gaps_query* __restrict__ queries, uint32_t n_queries, pgpu_factor* __restrict__ out_exons,
                 uint8_t* __restrict__ out_steps, pgpu_gaps_result* __restrict__ out) {
  __shared__ GapsLds S;
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_queries; c += gridDim.x) {
    const pgpu_gaps_query q = queries[c];
    const uint8_t* const est = ests + q.est_off;
    const uint32_t ne = q.n_exons;
    bool refused = ne > MAX_EXONS;
    __syncthreads();                                           // the query before is done with the LDS
    if (!refused && lane < ne) { S.ex[lane] = exons[q.first_exon + lane]; S.steps[lane] = 0; }
    __syncthreads();
    if (!refused) {                                            // the cap on an EST gap, before any gap is touched
      bool longer = false;
      if (lane + 1 < ne) longer = S.ex[lane + 1].EST_start - S.ex[lane].EST_end - 1 > (int)MAX_EST_GAP;
      refused = __any(longer);
    }
    // ---- the border loop (:1475-1514).  A gap writes the four ends that face it and reads the two ends of its donor and
    // the two starts of its acceptor: what it reads is the input's, whatever the gaps in front of it did
    uint32_t total = 0;
    for (uint32_t i = 0; i + 1 < ne && !refused; ++i) {
      const int d_est_end = __builtin_amdgcn_readfirstlane(S.ex[i].EST_end), d_gen_end = __builtin_amdgcn_readfirstlane(S.ex[i].GEN_end);
      const int a_est_start = __builtin_amdgcn_readfirstlane(S.ex[i + 1].EST_start);
      const int a_gen_start = __builtin_amdgcn_readfirstlane(S.ex[i + 1].GEN_start);
      const uint32_t gap_p = (uint32_t)(a_est_start - d_est_end - 1), gap_t = (uint32_t)(a_gen_start - d_gen_end - 1);
      if (gap_p == 0) continue;
      DevJob job;
      job.a = est + (d_est_end + 1); job.la = gap_p;
      job.b = T + (d_gen_end + 1); job.lb = gap_t;
      job.p0 = 0; job.p1 = job.p2 = gap_p; job.tail = 0;
      job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 1;
      lev_wave_body<1, MODE_BORDERS>(job, &S.res, nullptr, lane, S.rowmin);
      __syncthreads();                                         // lane 0's answer, for every lane
      // (v[0], the refusal of :1508, is always 1: the total is at most the pattern's length, which is max_errs)
      const uint32_t off_p = (uint32_t)__builtin_amdgcn_readfirstlane(S.res.v[1]), off_t1 = (uint32_t)__builtin_amdgcn_readfirstlane(S.res.v[2]);
      const uint32_t off_t2 = (uint32_t)__builtin_amdgcn_readfirstlane(S.res.v[3]), ed = (uint32_t)__builtin_amdgcn_readfirstlane(S.res.v[4]);
      total += ed;
      if (lane == 0) {                                         // :1502-1506
        S.ex[i].EST_end = d_est_end + (int)off_p;
        S.ex[i + 1].EST_start = d_est_end + (int)off_p + 1;
        S.ex[i].GEN_end = d_gen_end + (int)off_t1;
        S.ex[i + 1].GEN_start = a_gen_start - (int)(gap_t - off_t2);
        S.steps[i + 1] = (uint8_t)(1u + ed);
      }
      __syncthreads();                                         // read before the next gap's answer lands; the ends as moved
    }
    const uint32_t verdict = total > PGPU_GAPS_MAX_ERRORS ? 1u : 0u;
    // ---- the merging loop (:1522-1542): an exon within 3 genomic bytes of the running donor gives it its two ends
    if (!refused && verdict == 0 && lane == 0) {
      uint32_t dn = 0;
      for (uint32_t i = 1; i < ne; ++i) {
        if (S.ex[i].GEN_start - S.ex[dn].GEN_end - 1 <= 3) {
          S.ex[dn].EST_end = S.ex[i].EST_end; S.ex[dn].GEN_end = S.ex[i].GEN_end;
          S.steps[i] |= 0x80u;
        } else {
          dn = i;
        }
      }
    }
    __syncthreads();
    pgpu_gaps_result gr;
    gr.status = PGPU_OK; gr.verdict = verdict; gr.total_edit = total; gr.n_kept = 0;
    if (refused) { gr.status = PGPU_ERANGE; gr.verdict = 0; gr.total_edit = 0; }
    else {
      const bool merged = lane < ne && (S.steps[lane] & 0x80u) != 0;
      const uint32_t n_merged = (uint32_t)__popcll(__ballot(merged));
      if (verdict == 0) gr.n_kept = ne - n_merged;
      if (lane < ne) { out_exons[q.first_exon + lane] = S.ex[lane]; out_steps[q.first_exon + lane] = S.steps[lane]; }
    }
    if (lane == 0) out[c] = gr;
  }
}

thread_local double t_gaps_ms = 0.0;

}  // namespace

void pgpu_gaps_launch(const uint8_t* T, const uint8_t* ests, const pgpu_factor* exons, const pgpu_gaps_query* q, uint32_t n,
                      size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_gaps_result* out, hipStream_t st) {
  hipLaunchKernelGGL(gaps_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, ests, exons, q, n, out_exons, out_steps, out);
}

extern "C" double pgpu_index_gap_chains_kernel_ms(void) { return t_gaps_ms; }

extern "C" int pgpu_index_gap_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                     const pgpu_factor* exons, size_t n_exons_total, const pgpu_gaps_query* q, size_t n,
                                     pgpu_factor* out_exons, uint8_t* out_steps, pgpu_gaps_result* out) {
  t_gaps_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_gaps_query) == 24 && sizeof(pgpu_gaps_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, "queries", named);
  if (begun != CHAINED_GO) return begun;
  const auto own = [](const pgpu_gaps_query& x, const pgpu_factor* ex) { return gaps_query_ok(x, ex); };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, pgpu_index_length(idx), named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad gaps query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two "
                                           "queries share, a coordinate outside what it indexes, two adjacent exons out of order, "
                                           "or an EST gap longer than its genomic gap)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "gap chains");
  size_t waves = 0, cus = 0;
  TRY_HIP(chained_waves(n, waves, cus));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 0, 0);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(call.record(0));
  pgpu_gaps_launch(pgpu_index_genomic(idx), call.d, (const pgpu_factor*)(call.d + L.exons), (const pgpu_gaps_query*)(call.d + L.queries),
                   (uint32_t)n, waves, (pgpu_factor*)(call.d + L.out_exons), call.d + L.out_bytes,
                   (pgpu_gaps_result*)(call.d + L.results), call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_steps, out));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_gaps_ms);
  return PGPU_OK;
}
