// A candidate taken through clean, gaps and refine on the device, nothing leaving HBM in between.  Semantics:
// include/pintron_gpu.h (pgpu_pairing_plan_run_factorizations, pgpu_index_factorizations).
//
// Query c is EST c at every stage.  The three stage kernels are the ones of the chained entries, launched through
// pgpu_stage_launch.h and unchanged; an EST with nothing to do at a stage runs that stage's trivial query on a placeholder
// exon of its own (entry n_exons_total + c of every exon array), so there is no list of queries to compact, no count the
// host has to read between two stages, and no exon two waves could write.  Between the stages, one thread per EST:
//
//   fact_to_clean_kernel      the candidate (a query of the index form, or the plan's offsets and pgpu_cand_result) becomes
//                             a clean query.  What pgpu_index_clean_chains' validator refuses for a whole call is tested per
//                             EST (factor_ok, clean_query_need: the code of that entry) and is outcome HOST; the same pass
//                             folds the workspace the candidate's end-exon alignments need into two words (atomicMax).
//   fact_clean_to_gaps_kernel clean's result: PGPU_ERANGE is HOST, a verdict EMPTY, else the kept run of clean's out_exons,
//                             in place, is the gaps query, once gaps_query_ok (the code of pgpu_index_gap_chains) has passed.
//   fact_gaps_to_refine_kernel gaps' result likewise; the exons without bit 7 of their step byte are copied downwards into a
//                             second array from the same first index, tested for refine's precondition, and named by a
//                             chain query with the call's four settings.
//   fact_gather_kernel<false> refine's result: the outcome and the exon count for the scan (pgpu_exclusive_scan_u32);
//   fact_gather_kernel<true>  the exons and step bytes, compact, in EST order.
//
// These kernels read records of 16 to 40 bytes per thread and a handful of exons behind an index: no LDS, no per-thread
// array, no stack frame.  The one host wait of a call reads the two workspace words before clean_kernel is launched: the
// workspace of a wave is sized by the call's longest end exon (pgpu_clean.hip), up to 266 KB, and the grid by that size.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_gaps.h"
#include "pgpu_stage_launch.h"
#include "pgpu_stage_drive.h"
#include "pgpu_fact.h"

namespace {

constexpr uint32_t FACT_PENDING = 3u;      // outcome while the EST is on its way: never leaves the device

__device__ __forceinline__ pgpu_factor placeholder_exon() { pgpu_factor f; f.EST_start = f.EST_end = f.GEN_start = f.GEN_end = -1; return f; }
__device__ __forceinline__ void settle(pgpu_fact_result& r, uint32_t outcome, uint32_t stage, uint32_t detail) {
  r.outcome = (uint8_t)outcome; r.stage = (uint8_t)stage; r.detail = (uint16_t)detail;
}

__global__ __launch_bounds__(256)
void fact_to_clean_kernel(const pgpu_fact_query* __restrict__ fq, const unsigned long long* __restrict__ pat_off,
                          const pgpu_cand_result* __restrict__ cand, uint32_t n, uint32_t n_exons_total, uint32_t tlen,
                          double complexity_threshold, pgpu_factor* __restrict__ ex_in, pgpu_factor* __restrict__ ex_clean,
                          pgpu_clean_query* __restrict__ cq, pgpu_fact_result* __restrict__ res, uint32_t* __restrict__ need) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pgpu_clean_query q;
  q.reserved = 0; q.complexity_threshold = complexity_threshold;
  uint32_t kind;
  if (fq) {
    const pgpu_fact_query x = fq[i];
    q.est_off = x.est_off; q.est_len = x.est_len; q.first_exon = x.first_exon; q.n_exons = x.n_exons;
    kind = x.n_exons ? PGPU_CAND_ONE : PGPU_CAND_NONE;
  } else {
    const unsigned long long a = pat_off[i], b = pat_off[i + 1];
    const pgpu_cand_result c = cand[i];
    q.est_off = a; q.est_len = (uint32_t)(b - a); q.first_exon = c.first_exon; q.n_exons = c.n_exons;
    kind = c.kind;
  }
  pgpu_fact_result r;
  r.outcome = (uint8_t)FACT_PENDING; r.stage = 0; r.detail = 0; r.first_exon = 0; r.n_exons = 0; r.n_merged = 0; r.total_edit = 0;
  if (kind != PGPU_CAND_ONE) settle(r, kind == PGPU_CAND_REFUSED ? PGPU_FACT_EMPTY : PGPU_FACT_HOST, 0, kind);
  else if (q.n_exons > n_exons_total || q.first_exon > n_exons_total - q.n_exons) settle(r, PGPU_FACT_HOST, 1, 2);   // (a guard: neither form hands such a range in)
  else {
    const pgpu_factor* const ex = ex_in + q.first_exon;
    bool ok = true;
    for (uint32_t k = 0; k < q.n_exons && ok; ++k) ok = factor_ok(ex[k], q.est_len, tlen);
    size_t dirs = CLEAN_WS_DIRS_MIN, rows = CLEAN_WS_ROWS_MIN;
    if (ok) ok = clean_query_need(ex, q.n_exons, q.est_len, tlen, dirs, rows);
    if (!ok) settle(r, PGPU_FACT_HOST, 1, 2);
    else {
      if (dirs > CLEAN_WS_DIRS_MIN) atomicMax(need, (uint32_t)dirs);
      if (rows > CLEAN_WS_ROWS_MIN) atomicMax(need + 1, (uint32_t)rows);
    }
  }
  const uint32_t own = n_exons_total + i;
  ex_in[own] = placeholder_exon(); ex_clean[own] = placeholder_exon();
  if (r.outcome != FACT_PENDING) { q.first_exon = own; q.n_exons = 1; }      // verdict 1 at step 1, before any alignment
  cq[i] = q;
  res[i] = r;
}

__global__ __launch_bounds__(256)
void fact_clean_to_gaps_kernel(const pgpu_clean_query* __restrict__ cq, const pgpu_clean_result* __restrict__ cr, uint32_t n,
                               uint32_t n_exons_total, const pgpu_factor* __restrict__ ex_clean, pgpu_gaps_query* __restrict__ gq,
                               pgpu_fact_result* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgpu_clean_query c = cq[i];
  pgpu_gaps_query q;
  q.est_off = c.est_off; q.est_len = c.est_len; q.first_exon = n_exons_total + i; q.n_exons = 1; q.reserved = 0;   // verdict 0, no DP
  pgpu_fact_result r = res[i];
  if (r.outcome == FACT_PENDING) {
    const pgpu_clean_result a = cr[i];
    if (a.status != PGPU_OK) settle(r, PGPU_FACT_HOST, 1, 1);
    else if (a.verdict != 0) settle(r, PGPU_FACT_EMPTY, 1, a.verdict);
    else {
      pgpu_gaps_query g = q;
      g.first_exon = c.first_exon + a.first_kept; g.n_exons = a.n_kept;
      if (!gaps_query_ok(g, ex_clean + g.first_exon)) settle(r, PGPU_FACT_HOST, 2, 2);
      else q = g;
    }
    res[i] = r;
  }
  gq[i] = q;
}

__global__ __launch_bounds__(256)
void fact_gaps_to_refine_kernel(const pgpu_gaps_query* __restrict__ gq, const pgpu_gaps_result* __restrict__ gr, uint32_t n,
                                uint32_t n_exons_total, const pgpu_factor* __restrict__ ex_gaps, const uint8_t* __restrict__ gsteps,
                                pgpu_fact_params prm, pgpu_factor* __restrict__ ex_kept, pgpu_chain_query* __restrict__ rq,
                                pgpu_fact_result* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgpu_gaps_query g = gq[i];
  pgpu_chain_query q;
  q.est_off = g.est_off; q.est_len = g.est_len; q.first_exon = n_exons_total + i; q.n_exons = 1; q.reserved = 0;   // done 0
  q.suffpref_length_on_est = prm.suffpref_length_on_est; q.suffpref_length_for_intron = prm.suffpref_length_for_intron;
  q.suffpref_length_on_gen = prm.suffpref_length_on_gen; q.min_intron_length = prm.min_intron_length;
  ex_kept[n_exons_total + i] = placeholder_exon();
  pgpu_fact_result r = res[i];
  if (r.outcome == FACT_PENDING) {
    const pgpu_gaps_result a = gr[i];
    if (a.status != PGPU_OK) settle(r, PGPU_FACT_HOST, 2, 1);
    else {
      r.total_edit = a.total_edit;
      if (a.verdict != 0) settle(r, PGPU_FACT_EMPTY, 2, 1);
      else {
        // the exons check_gap_errors kept, moved down: the donors hold their merged ends already
        uint32_t kept = 0;
        bool ordered = true;
        pgpu_factor prev = placeholder_exon();
        for (uint32_t k = 0; k < g.n_exons; ++k) {
          if (gsteps[g.first_exon + k] & 0x80u) continue;
          const pgpu_factor f = ex_gaps[g.first_exon + k];
          if (kept && !(prev.EST_end < f.EST_start && prev.GEN_end < f.GEN_start)) ordered = false;
          ex_kept[g.first_exon + kept] = f;
          prev = f; ++kept;
        }
        if (!ordered) settle(r, PGPU_FACT_HOST, 3, 2);
        else { q.first_exon = g.first_exon; q.n_exons = kept; r.n_merged = (uint16_t)(g.n_exons - kept); }
      }
    }
    res[i] = r;
  }
  rq[i] = q;
}

template <bool WRITE>
__global__ __launch_bounds__(256)
void fact_gather_kernel(const pgpu_chain_query* __restrict__ rq, const pgpu_chain_result* __restrict__ rr, uint32_t n,
                        pgpu_fact_result* __restrict__ res, uint32_t* __restrict__ counts,
                        const unsigned long long* __restrict__ first, const pgpu_factor* __restrict__ ex_refined,
                        const uint8_t* __restrict__ rsteps, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pgpu_fact_result r = res[i];
  if (WRITE) {
    if (r.outcome != PGPU_FACT_DONE) return;
    const unsigned long long at = first[i];
    const uint32_t from = rq[i].first_exon + (r.detail & 1u);
    for (uint32_t k = 0; k < r.n_exons; ++k) {
      out_exons[at + k] = ex_refined[from + k];
      out_steps[at + k] = (k == 0 && !(r.detail & 1u)) ? (uint8_t)0 : rsteps[from + k];      // chain_kernel writes no byte for a first exon
    }
    res[i].first_exon = (uint32_t)at;
    return;
  }
  if (r.outcome == FACT_PENDING) {
    const pgpu_chain_result a = rr[i];
    if (a.status != PGPU_OK) { settle(r, PGPU_FACT_HOST, 3, 1); r.n_merged = 0; }
    else {
      settle(r, PGPU_FACT_DONE, 3, a.dropped_first ? 1u : 0u);
      r.n_exons = (uint16_t)(rq[i].n_exons - (a.dropped_first ? 1u : 0u));
    }
    res[i] = r;
  }
  counts[i] = r.outcome == PGPU_FACT_DONE ? r.n_exons : 0u;
}

thread_local double t_fact_ms = 0.0;

}  // namespace

hipError_t pgpu_fact_drive(pgpu_ctx* ctx, pgpu_fact_job& d, const pgpu_fact_params& prm) {
  const uint32_t n = d.n, E = d.n_exons_total;
  const FactLayout L = fact_layout(n, E, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  pgpu_factor* const ex_in = (pgpu_factor*)(B + L.ex_in);
  pgpu_factor* const ex_clean = (pgpu_factor*)(B + L.ex_clean);
  pgpu_factor* const ex_gaps = (pgpu_factor*)(B + L.ex_gaps);
  pgpu_factor* const ex_kept = (pgpu_factor*)(B + L.ex_kept);
  pgpu_factor* const ex_refined = (pgpu_factor*)(B + L.ex_refined);
  pgpu_clean_query* const cq = (pgpu_clean_query*)(B + L.cq);
  pgpu_clean_result* const cr = (pgpu_clean_result*)(B + L.cr);
  pgpu_gaps_query* const gq = (pgpu_gaps_query*)(B + L.gq);
  pgpu_gaps_result* const gr = (pgpu_gaps_result*)(B + L.gr);
  pgpu_chain_query* const rq = (pgpu_chain_query*)(B + L.rq);
  pgpu_chain_result* const rr = (pgpu_chain_result*)(B + L.rr);
  pgpu_fact_result* const res = (pgpu_fact_result*)(B + L.res);
  uint32_t* const need = (uint32_t*)(B + L.need);                  // ws_dirs, ws_rows, clean's `undersized` flag
  uint32_t* const counts = (uint32_t*)(B + L.counts);
  unsigned long long* const first = (unsigned long long*)(B + L.first);
  const dim3 grid((n + 255) / 256), blk(256);
  d.total = 0; d.undersized = 0;

  DRIVE(drive_record(d.ev, 0, st));
  const uint32_t need0[3] = { CLEAN_WS_DIRS_MIN, CLEAN_WS_ROWS_MIN, 0 };
  DRIVE(hipMemcpyAsync(need, need0, sizeof need0, hipMemcpyHostToDevice, st));
  if (E && d.cand_exons != ex_in) DRIVE(hipMemcpyAsync(ex_in, d.cand_exons, (size_t)E * sizeof(pgpu_factor), hipMemcpyDeviceToDevice, st));
  if (E) DRIVE(hipMemcpyAsync(ex_clean, ex_in, (size_t)E * sizeof(pgpu_factor), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(fact_to_clean_kernel, grid, blk, 0, st, d.fq, d.pat_off, d.cand, n, E, d.tlen, prm.complexity_threshold, ex_in,
                     ex_clean, cq, res, need);
  // the one host wait inside the call: what the end-exon alignments of this call need of a wave's workspace
  uint32_t sized[2] = { 0, 0 };
  DRIVE(hipMemcpyAsync(sized, need, sizeof sized, hipMemcpyDeviceToHost, st));
  DRIVE(pgpu_ctx_wait(ctx));
  DRIVE(hipGetLastError());
  const size_t ws_dirs = sized[0], ws_rows = sized[1];
  size_t waves_clean = 0, ws_wave_clean = 0, waves = 0, cus = 0;
  DRIVE(pgpu_clean_grid(n, ws_dirs, ws_rows, waves_clean, ws_wave_clean));
  DRIVE(chained_waves(n, waves, cus));
  // clean's and refine's workspaces are never live together: one block for both
  const size_t ws_clean = waves_clean * ws_wave_clean, ws_chain = waves * pgpu_chain_ws_wave();
  uint8_t* const ws = (uint8_t*)d.ws_alloc(d.ws_user, ws_clean > ws_chain ? ws_clean : ws_chain);
  if (!ws) return hipErrorOutOfMemory;

  DRIVE(drive_record(d.ev, 2, st));
  pgpu_clean_launch(d.T, d.tlen, d.ests, ex_in, cq, n, ws, ws_dirs, ws_rows, waves_clean, ex_clean, B + L.marks, cr, need + 2, st);
  DRIVE(drive_record(d.ev, 3, st));
  hipLaunchKernelGGL(fact_clean_to_gaps_kernel, grid, blk, 0, st, cq, cr, n, E, ex_clean, gq, res);
  DRIVE(drive_record(d.ev, 4, st));
  pgpu_gaps_launch(d.T, d.ests, ex_clean, gq, n, waves, ex_gaps, B + L.gsteps, gr, st);
  DRIVE(drive_record(d.ev, 5, st));
  hipLaunchKernelGGL(fact_gaps_to_refine_kernel, grid, blk, 0, st, gq, gr, n, E, ex_gaps, B + L.gsteps, prm, ex_kept, rq, res);
  DRIVE(drive_record(d.ev, 6, st));
  pgpu_chain_launch(d.T, d.tlen, d.ests, ex_kept, rq, n, ws, waves, ex_refined, B + L.rsteps, rr, st);
  DRIVE(drive_record(d.ev, 7, st));
  hipLaunchKernelGGL(fact_gather_kernel<false>, grid, blk, 0, st, rq, rr, n, res, counts, (const unsigned long long*)nullptr,
                     (const pgpu_factor*)nullptr, (const uint8_t*)nullptr, (pgpu_factor*)nullptr, (uint8_t*)nullptr);
  DRIVE(drive_scan(counts, first, n, B + L.scan_tmp, st));
  hipLaunchKernelGGL(fact_gather_kernel<true>, grid, blk, 0, st, rq, rr, n, res, (uint32_t*)nullptr, first, ex_refined, B + L.rsteps,
                     (pgpu_factor*)(B + L.out_exons), B + L.out_steps);
  DRIVE(drive_record(d.ev, 1, st));
  DRIVE(hipMemcpyAsync(&d.total, first + n, sizeof d.total, hipMemcpyDeviceToHost, st));       // drive_total written out:
  DRIVE(hipMemcpyAsync(&d.undersized, need + 2, sizeof d.undersized, hipMemcpyDeviceToHost, st));      // a second word comes back
  DRIVE(pgpu_ctx_wait(ctx));
  return hipGetLastError();
}

extern "C" double pgpu_index_factorizations_kernel_ms(void) { return t_fact_ms; }

extern "C" int pgpu_index_factorizations(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                         const pgpu_factor* exons, size_t n_exons_total, const pgpu_fact_query* q, size_t n,
                                         const pgpu_fact_params* params, pgpu_fact_result* out, pgpu_factor* out_exons,
                                         uint8_t* out_steps, size_t cap, size_t* n_out) {
  t_fact_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_fact_query) == 24 && sizeof(pgpu_fact_params) == 24 && sizeof(pgpu_fact_result) == 16, "ABI layout");
  if (!ctx || !idx || !params || !n_out || (n && (!q || !out)) || (ests_len && !ests) || (n_exons_total && !exons) ||
      (cap && (!out_exons || !out_steps)))
    return PGPU_EINVAL;
  if (n > 0x7fffffffull || n_exons_total > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, FACT_TOO_MANY);
  if (!fact_params_ok(*params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, FACT_BAD_PARAMS);
  NamedExons named;
  named.p = (uint8_t*)calloc(n_exons_total ? n_exons_total : 1, 1);
  if (!named.p) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "no memory for the table of the exons the queries name");
  if (!fact_queries_ok(q, n, ests_len, n_exons_total, named.p))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad factorization query (a range past its buffer, an empty EST, reserved != 0, or an exon "
                                           "two queries share)");
  *n_out = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "factorizations");
  // the one device block: [ests + 64 | queries | the driver's block]; the workspace in a second one, once it is sized
  const FactLayout L = fact_layout(n, n_exons_total, pgpu_scan_tmp_bytes(n + 1));
  BlockCarver c{up256(ests_len + 64)};
  const size_t o_q = c.take(n * sizeof *q), o_block = c.take(L.total);
  TRY_HIP(hipMalloc((void**)&call.d, c.at));
  TRY_HIP(call.timing_events(4));
  if (ests_len) TRY_HIP(hipMemcpyAsync(call.d, ests, ests_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_q, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  pgpu_fact_job job;
  TRY_HIP(pgpu_fact_index_job(call, idx, o_q, o_block, exons, n_exons_total, n, job));
  TRY_HIP(pgpu_fact_drive(ctx, job, *params));
  if (job.undersized) return pgpu_clean_undersized(ctx, "factorizations");
  *n_out = (size_t)job.total;
  if (job.total > cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  TRY_HIP(drive_download(job.block, L, n * sizeof *out, job.total, out, out_exons, out_steps, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  call.elapsed_ms(0, &t_fact_ms);
  return PGPU_OK;
}

hipError_t pgpu_fact_index_job(QueryCall& call, const pgpu_index* idx, size_t o_fq, size_t o_block, const pgpu_factor* exons,
                               size_t n_exons_total, size_t n, pgpu_fact_job& job) {
  job.T = pgpu_index_genomic(idx); job.tlen = (uint32_t)pgpu_index_length(idx); job.ests = call.d;
  job.fq = (const pgpu_fact_query*)(call.d + o_fq); job.pat_off = nullptr; job.cand = nullptr;
  job.n = (uint32_t)n; job.n_exons_total = (uint32_t)n_exons_total; job.block = call.d + o_block;
  uint8_t* const ex_in = job.block + fact_layout(n, n_exons_total, pgpu_scan_tmp_bytes(n + 1)).ex_in;
  job.cand_exons = (const pgpu_factor*)ex_in;          // uploaded where the driver wants them
  job.ws_alloc = [](void* user, size_t bytes) -> void* {
    QueryCall* c = (QueryCall*)user;
    return hipMalloc((void**)&c->d2, bytes ? bytes : 16) == hipSuccess ? c->d2 : nullptr;
  };
  job.ws_user = &call;
  for (int k = 0; k < 8; ++k) job.ev[k] = call.ev[k];
  return n_exons_total ? hipMemcpyAsync(ex_in, exons, n_exons_total * sizeof(pgpu_factor), hipMemcpyHostToDevice, call.st) : hipSuccess;
}
