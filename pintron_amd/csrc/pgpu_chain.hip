// All of refine_intron, chained per EST, on the resident index.  Semantics: include/pintron_gpu.h
// (pgpu_index_refine_chains): one query is one factorization, and the answer is the factorization as the loop of
// src/est-factorizations.c:446-490 leaves it.
//
//   chain_kernel    one wave per chain; a wave that has finished a chain takes the next one of its stride.  Per intron,
//                   in chain order and without the host in between:
//                     windows    the real_substring pieces of src/refine-intron.c:55-116 (ef_gap_window_build's clamping)
//                                cut from the uploaded ESTs and the resident genomic into the wave's workspace;
//                     alignment  gap_wave_body<R> and gap_traceback_wave of pgpu_wave_dp.h on a DevJob built here: the code
//                                of the PGPU_DP_GAP jobs of a plan, with the row class the plan builder would choose;
//                     decision   refine_decide of pgpu_refine_body.h on the rows staged in LDS: the code of refine_kernel.
//                   The acceptor the decision leaves is the donor of the next intron and stays in registers.  Divergence
//                   is per chain: everything that decides is uniform over the wave.
//                   The direction bytes (one per cell, step-major as gap_wave_body writes them: up to 96 KB at the caps)
//                   live in a per-wave workspace in HBM, as for gap_wave in a plan; the traceback's window and the
//                   decision's buffers share the wave's LDS, for they are never live together.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_wave_dp.h"
#include "pgpu_refine_body.h"
#include "pgpu_stage_launch.h"

namespace {

constexpr int MAX_EW = PGPU_CHAIN_MAX_EST_WINDOW;
constexpr int MAX_GW = PGPU_CHAIN_MAX_GEN_WINDOW;
constexpr uint32_t CHAIN_R = 4;                        // row class of the longest EST window
static_assert(MAX_EW <= 64 * (int)CHAIN_R && MAX_EW + MAX_GW <= MAX_DIM, "the caps fit the sweep and the decision");

// the workspace of one wave: direction bytes as ws_gap of the plan builder sizes them, the two gapped strings, the two
// windows, the alignment's result
constexpr size_t WS_DIRS = ((size_t)MAX_GW + 64) * 64 * CHAIN_R;
constexpr size_t WS_STRS = WS_DIRS;
constexpr size_t WS_STRS_BYTES = (2 * ((size_t)MAX_EW + MAX_GW + 1) + 15) & ~(size_t)15;
constexpr size_t WS_WIN_E = WS_STRS + WS_STRS_BYTES;
constexpr size_t WS_WIN_G = WS_WIN_E + ((MAX_EW + 15) & ~15);
constexpr size_t WS_RES = WS_WIN_G + ((MAX_GW + 15) & ~15);
constexpr size_t WS_WAVE = (WS_RES + sizeof(DevResult) + 255) & ~(size_t)255;

// LDS of one wave: the traceback's direction window and path, then (the traceback over) what the decision stages
struct ChainLds {
  union {
    struct { __attribute__((aligned(16))) uint8_t win[TB_WIN_BYTES]; uint8_t path[TB_PATH]; } tb;
    RefineLds refine;
  };
};

// appends real_substring(index, length) of s to dst[at ..) when it fits `cap`; returns the new length (beyond cap: nothing
// more is written, the caller refuses the intron)
__device__ __forceinline__ int append_piece(uint8_t* dst, int at, int cap, const Seq& s, int index, int length, int lane) {
  if (at > cap) return at;
  // no piece is scanned for its terminator beyond the first byte that would not fit: a length of 2^24 gets the same
  // verdict as cap + 1.  The negative index shortens the piece first, as substring() would.
  if (index < 0) { length += index; index = 0; }
  if (length > cap - at + 1) length = cap - at + 1;
  const Piece p = substring(s, index, length, lane);
  if (p.len > cap - at) return cap + 1;
  for (int k = lane; k < p.len; k += 64) dst[at + k] = s.p[p.start + k];
  return at + p.len;
}

__global__ __launch_bounds__(64)
void chain_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint8_t* __restrict__ ests, const pgpu_factor* __restrict__ exons,
                  const pgpu_chain_query* __restrict__ queries, uint32_t n_chains, uint8_t* __restrict__ ws,
                  pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps, pgpu_chain_result* __restrict__ out) {
  __shared__ ChainLds S;
  const int lane = (int)threadIdx.x;
  uint8_t* const w = ws + (size_t)blockIdx.x * WS_WAVE;
  uint8_t* const win_e = w + WS_WIN_E;
  uint8_t* const win_g = w + WS_WIN_G;
  DevResult* const res = reinterpret_cast<DevResult*>(w + WS_RES);
  for (uint32_t c = blockIdx.x; c < n_chains; c += gridDim.x) {
    const pgpu_chain_query q = queries[c];
    Seq est, gen;
    est.p = ests + q.est_off; est.len = (int)q.est_len;
    gen.p = T; gen.len = (int)n;
    const int sp_est = q.suffpref_length_on_est, sp_int = q.suffpref_length_for_intron, sp_gen = q.suffpref_length_on_gen;
    pgpu_chain_result cr;
    cr.status = PGPU_OK; cr.done = 0; cr.dropped_first = 0; cr.pad = 0;
    pgpu_factor donor = exons[q.first_exon];
    const int first_est_start = donor.EST_start;
    int second_est_start = 0;
    uint32_t i = 0;
    for (; i + 1 < q.n_exons; ++i) {
      const pgpu_factor acceptor = exons[q.first_exon + i + 1];
      // the windows (:55-116)
      int dsl_gen = donor.GEN_start;
      if (donor.GEN_end - sp_gen + 1 >= dsl_gen) dsl_gen = donor.GEN_end - sp_gen + 1;
      int dsl_est = donor.EST_start;
      if (donor.EST_end - sp_est + 1 >= dsl_est) dsl_est = donor.EST_end - sp_est + 1;
      int apr_gen = acceptor.GEN_end;
      if (acceptor.GEN_start + sp_gen - 1 <= apr_gen) apr_gen = acceptor.GEN_start + sp_gen - 1;
      int apr_est = acceptor.EST_end;
      if (acceptor.EST_start + sp_est - 1 <= apr_est) apr_est = acceptor.EST_start + sp_est - 1;
      int le = 0, lg = 0;
      le = append_piece(win_e, le, MAX_EW, est, dsl_est, donor.EST_end - dsl_est + 1, lane);
      if (donor.EST_end != acceptor.EST_start - 1)
        le = append_piece(win_e, le, MAX_EW, est, donor.EST_end + 1, acceptor.EST_start - donor.EST_end - 1, lane);
      le = append_piece(win_e, le, MAX_EW, est, acceptor.EST_start, apr_est - acceptor.EST_start + 1, lane);
      lg = append_piece(win_g, lg, MAX_GW, gen, dsl_gen, donor.GEN_end - dsl_gen + 1, lane);
      lg = append_piece(win_g, lg, MAX_GW, gen, donor.GEN_end + 1, sp_int, lane);
      lg = append_piece(win_g, lg, MAX_GW, gen, acceptor.GEN_start - sp_int, sp_int, lane);
      lg = append_piece(win_g, lg, MAX_GW, gen, acceptor.GEN_start, apr_gen - acceptor.GEN_start + 1, lane);
      if (le > MAX_EW || lg > MAX_GW) { cr.status = PGPU_ERANGE; break; }
      // the gap alignment (:560-890) as a PGPU_DP_GAP job
      DevJob job;
      job.a = win_e; job.b = win_g; job.la = (uint32_t)le; job.lb = (uint32_t)lg;
      job.p0 = job.p1 = job.p2 = job.tail = 0;
      job.ws_off = 0; job.str_off = WS_STRS; job.out_idx = 0;
      job.r_class = le <= 64 ? 1u : (le <= 128 ? 2u : 4u);
      own_stores_visible();                  // the windows
      switch (job.r_class) {
        case 1:  gap_wave_body<1>(job, res, w, (uint32_t)lane); break;
        case 2:  gap_wave_body<2>(job, res, w, (uint32_t)lane); break;
        default: gap_wave_body<4>(job, res, w, (uint32_t)lane); break;
      }
      own_stores_visible();                  // the planes and the start plane (res->pad)
      gap_traceback_wave(job, res, w, w, (uint32_t)lane, S.tb.win, S.tb.path);
      own_stores_visible();                  // the two strings and the five values
      // the decision (:118-257) on the rows in LDS
      pgpu_refine_query rq;
      rq.est_off = q.est_off; rq.est_len = q.est_len; rq.flags = i == 0 ? PGPU_REFINE_FIRST_INTRON : 0u;
      rq.rows_off = 0; rq.dim = (uint32_t)__builtin_amdgcn_readfirstlane(res->v[0]);
      rq.factor_cut = __builtin_amdgcn_readfirstlane(res->v[1]);
      rq.intron_start = __builtin_amdgcn_readfirstlane(res->v[2]);
      rq.intron_end = __builtin_amdgcn_readfirstlane(res->v[3]);
      rq.intron_start_on_align = __builtin_amdgcn_readfirstlane(res->v[4]);
      rq.intron_end_on_align = __builtin_amdgcn_readfirstlane(res->v[5]);
      rq.donor = donor; rq.acceptor = acceptor;
      rq.suffpref_length_on_est = sp_est; rq.suffpref_length_for_intron = sp_int; rq.suffpref_length_on_gen = sp_gen;
      rq.min_intron_length = q.min_intron_length;
      const int dim = (int)rq.dim;                             // <= MAX_EW + MAX_GW <= MAX_DIM
      const uint8_t* const row_e = w + (uint32_t)__builtin_amdgcn_readfirstlane((int)res->str[0]);
      const uint8_t* const row_g = w + (uint32_t)__builtin_amdgcn_readfirstlane((int)res->str[1]);
      __syncthreads();                                         // the traceback's window is dead: the decision takes its LDS
      for (int k = lane; k < dim; k += 64) { S.refine.rows[k] = row_e[k]; S.refine.rows[dim + k] = row_g[k]; }
      __syncthreads();
      pgpu_refine_result r;
      r.status = PGPU_OK; r.refined = 0; r.path = 0; r.pad = 0; r.donor = donor; r.acceptor = acceptor;
      refine_decide(S.refine, S.refine.rows, S.refine.rows + dim, dim, rq, T, n, ests, lane, r);
      __syncthreads();                                         // ... and gives it back
      if (r.status != PGPU_OK) { cr.status = PGPU_ERANGE; break; }
      if (lane == 0) {
        out_exons[q.first_exon + i] = r.donor;
        out_steps[q.first_exon + i + 1] = (uint8_t)((uint32_t)r.path | ((uint32_t)r.refined << 7));
      }
      if (i == 0) second_est_start = r.acceptor.EST_start;
      donor = r.acceptor;
    }
    cr.done = i;
    // the exon the chain stopped at, as it stands; behind a refusal the exons that follow stay the copies of the input
    if (lane == 0) out_exons[q.first_exon + i] = donor;
    // the first-exon rule (src/est-factorizations.c:476-485)
    if (cr.status == PGPU_OK && q.n_exons > 1 && first_est_start == second_est_start) cr.dropped_first = 1;
    if (lane == 0) out[c] = cr;
  }
}

thread_local double t_chain_ms = 0.0;

}  // namespace

size_t pgpu_chain_ws_wave(void) { return WS_WAVE; }

void pgpu_chain_launch(const uint8_t* T, uint32_t tlen, const uint8_t* ests, const pgpu_factor* exons, const pgpu_chain_query* q,
                       uint32_t n, uint8_t* ws, size_t waves, pgpu_factor* out_exons, uint8_t* out_steps, pgpu_chain_result* out,
                       hipStream_t st) {
  hipLaunchKernelGGL(chain_kernel, dim3((unsigned)waves), dim3(64), 0, st, T, tlen, ests, exons, q, n, ws, out_exons, out_steps, out);
}

extern "C" double pgpu_index_refine_chains_kernel_ms(void) { return t_chain_ms; }

extern "C" int pgpu_index_refine_chains(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                        const pgpu_factor* exons, size_t n_exons_total,
                                        const pgpu_chain_query* q, size_t n,
                                        pgpu_factor* out_exons, uint8_t* out_steps, pgpu_chain_result* out) {
  t_chain_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_chain_query) == 40 && sizeof(pgpu_chain_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  NamedExons named;
  const int begun = chained_begin(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, out_exons, out_steps, out, "chains", named);
  if (begun != CHAINED_GO) return begun;
  const size_t glen = pgpu_index_length(idx);
  // a chain's own rules: the suffpref lengths, and the my_asserts of :52-53, on fields no earlier step writes
  const auto own = [](const pgpu_chain_query& x, const pgpu_factor* ex) {
    bool ok = suffpref_ok(x.suffpref_length_on_est, x.suffpref_length_for_intron, x.suffpref_length_on_gen);
    for (uint32_t k = 0; ok && k + 1 < x.n_exons; ++k) ok = ex[k].EST_end < ex[k + 1].EST_start && ex[k].GEN_end < ex[k + 1].GEN_start;
    return ok;
  };
  if (!chained_queries_ok(q, n, ests_len, exons, n_exons_total, glen, named.p, own))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad chain query (a range past its buffer, reserved != 0, no exon, an exon two chains "
                                           "share, a donor that is not in front of its acceptor, or a coordinate outside what it "
                                           "indexes)");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "refine chains");
  size_t waves = 0, cus = 0;
  TRY_HIP(chained_waves(n, waves, cus));
  const ChainedLayout L = chained_layout(ests_len, n_exons_total, n, sizeof *q, sizeof *out, 0, waves * WS_WAVE);
  TRY_HIP(hipMalloc((void**)&call.d, L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(chained_upload(call, L, ests, exons, q));
  TRY_HIP(call.record(0));
  pgpu_chain_launch(pgpu_index_genomic(idx), (uint32_t)glen, call.d, (const pgpu_factor*)(call.d + L.exons),
                    (const pgpu_chain_query*)(call.d + L.queries), (uint32_t)n, call.d + L.ws, waves,
                    (pgpu_factor*)(call.d + L.out_exons), call.d + L.out_bytes, (pgpu_chain_result*)(call.d + L.results), call.st);
  TRY_HIP(call.record(1));
  TRY_HIP(chained_download(call, L, out_exons, out_steps, out));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  call.elapsed_ms(0, &t_chain_ms);
  return PGPU_OK;
}
