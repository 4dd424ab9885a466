// The refined exons of the factorization driver (pgpu_fact.hip) taken through the tail and the small stage on the device,
// nothing leaving HBM in between.  Semantics: include/pintron_gpu.h (pgpu_pairing_plan_run_final_factorizations,
// pgpu_index_final_factorizations).
//
// The input is the answer of pgpu_fact_drive where it lies: its outcomes, its compact exons.  Query c is EST c at both
// stages, as there.  The two stage kernels are the ones of the chained entries, launched through pgpu_stage_launch.h and
// unchanged; an EST with nothing to do at a stage runs that stage's trivial query on a placeholder exon of its own (entry
// n_exons_total + c of every input array).  Between the stages, one thread per EST:
//
//   final_to_tail_kernel        an outcome of the stages 0-3 that is not DONE is carried over; for DONE the refined exons are
//                               copied out of the compact array (from the same first index: the compact ranges share no
//                               entry) and named by a tail query, once tail_query_ok (the code of pgpu_index_tail_chains)
//                               has passed.
//   final_tail_to_small_kernel  tail's result: PGPU_ERANGE is HOST, verdict 1 EMPTY, else the exons step 5 did not remove are
//                               copied downwards into a second array from the same first index and named by a small query,
//                               once small_query_ok has passed.
//   final_gather_kernel<false>  small's result: the outcome and the exon count for the scan (pgpu_exclusive_scan_u32);
//   final_gather_kernel<true>   the kept run of small's list and its step bytes, compact, in EST order.
//
// These kernels read records of 16 to 32 bytes per thread and a handful of exons behind an index: no LDS, no per-thread
// array, no stack frame.  The one host wait of the drive is its last statement.
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_classify.h"
#include "pgpu_small.h"
#include "pgpu_stage_launch.h"
#include "pgpu_stage_drive.h"
#include "pgpu_final.h"

namespace {

constexpr uint32_t FINAL_PENDING = 3u;     // outcome while the EST is on its way: never leaves the device

__device__ __forceinline__ void settle(pgpu_final_result& r, uint32_t outcome, uint32_t stage, uint32_t detail) {
  r.outcome = (uint8_t)outcome; r.stage = (uint8_t)stage; r.detail = (uint16_t)detail;
}

__global__ __launch_bounds__(256)
void final_to_tail_kernel(const pgpu_final_query* __restrict__ fq, const unsigned long long* __restrict__ pat_off,
                          const unsigned long long* __restrict__ orig_off, const pgpu_fact_result* __restrict__ fres,
                          const pgpu_factor* __restrict__ fexons, uint32_t n, uint32_t n_exons_total, size_t ests_len, uint32_t tlen,
                          pgpu_factor* __restrict__ ex_tin, pgpu_tail_query* __restrict__ tq, pgpu_final_result* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t own = n_exons_total + i;
  pgpu_tail_query q;
  if (fq) { const pgpu_final_query x = fq[i]; q.est_off = x.est_off; q.est_len = x.est_len; q.orig_off = x.orig_off; }
  else { const unsigned long long a = pat_off[i]; q.est_off = a; q.est_len = (uint32_t)(pat_off[i + 1] - a); q.orig_off = orig_off[i]; }
  q.first_exon = own; q.n_exons = 1; q.reserved = 0;
  // (0, est_len - 1, 0, 0): no step of tail has anything to do.  An empty pattern of a plan (est_len == 0, never DONE) gets
  // (0, -1, 0, 0): steps 1 and 2 read nothing, step 3 says verdict 1, nobody reads it; small's (0, 0, 0, 0) then reads one
  // byte at est_off, inside the slack behind the sequences
  pgpu_factor trivial;
  trivial.EST_start = 0; trivial.EST_end = (int32_t)q.est_len - 1; trivial.GEN_start = 0; trivial.GEN_end = 0;
  ex_tin[own] = trivial;
  const pgpu_fact_result f = fres[i];
  pgpu_final_result r;
  r.outcome = f.outcome; r.stage = f.stage; r.detail = f.detail; r.first_exon = 0; r.n_exons = 0; r.n_merged = f.n_merged;
  r.total_edit = f.total_edit; r.tail_added = 0; r.polyA = r.polyadenil = r.recovered = r.refused = 0;
  r.n_removed = r.n_added = r.n_cleaned = 0; r.prefix_added = r.reserved = 0;
  if (f.outcome == PGPU_FACT_DONE) {
    pgpu_tail_query g = q;
    g.first_exon = f.first_exon; g.n_exons = f.n_exons;
    // (a guard: the driver hands no range in that leaves the compact array, which has n_exons_total entries)
    if (g.n_exons == 0 || g.n_exons > n_exons_total || g.first_exon > n_exons_total - g.n_exons) settle(r, PGPU_FACT_HOST, 4, 2);
    else {
      for (uint32_t k = 0; k < g.n_exons; ++k) ex_tin[g.first_exon + k] = fexons[g.first_exon + k];
      if (!tail_query_ok(g, ex_tin + g.first_exon, ests_len, tlen)) settle(r, PGPU_FACT_HOST, 4, 2);
      else { q = g; settle(r, FINAL_PENDING, 3, f.detail & 1u); }
    }
  }
  tq[i] = q;
  res[i] = r;
}

__global__ __launch_bounds__(256)
void final_tail_to_small_kernel(const pgpu_tail_query* __restrict__ tq, const pgpu_tail_result* __restrict__ tr, uint32_t n,
                                uint32_t n_exons_total, size_t ests_len, uint32_t tlen, const pgpu_factor* __restrict__ ex_tout,
                                const uint8_t* __restrict__ tsteps, pgpu_factor* __restrict__ ex_sin,
                                pgpu_small_query* __restrict__ sq, pgpu_final_result* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t own = n_exons_total + i;
  const pgpu_tail_query t = tq[i];
  pgpu_small_query q = t;
  q.first_exon = own; q.n_exons = 1;
  pgpu_factor trivial;                                  // (0, 0, 0, 0): no prefix to search, no pair, a cleaning of one cell
  trivial.EST_start = trivial.EST_end = trivial.GEN_start = trivial.GEN_end = 0;
  ex_sin[own] = trivial;
  pgpu_final_result r = res[i];
  if (r.outcome == FINAL_PENDING) {
    const pgpu_tail_result a = tr[i];
    if (a.status != PGPU_OK) settle(r, PGPU_FACT_HOST, 4, 1);
    else {
      r.tail_added = a.tail_added; r.polyA = a.polyA; r.polyadenil = a.polyadenil; r.recovered = a.recovered;
      if (a.verdict != 0) settle(r, PGPU_FACT_EMPTY, 4, 1);
      else {
        // the exons remove_false_small_exons kept, moved down: their neighbours hold the merged ends already
        uint32_t kept = 0;
        for (uint32_t k = 0; k < t.n_exons; ++k) {
          if ((tsteps[t.first_exon + k] & 3u) == 3u) continue;
          ex_sin[t.first_exon + kept] = ex_tout[t.first_exon + k];
          ++kept;
        }
        r.n_removed = (uint16_t)(t.n_exons - kept);
        pgpu_small_query g = t;
        g.n_exons = kept;
        if (kept == 0 || !small_query_ok(g, ex_sin + g.first_exon, ests_len, tlen)) settle(r, PGPU_FACT_HOST, 5, 2);
        else q = g;
      }
    }
    res[i] = r;
  }
  sq[i] = q;
}

template <bool WRITE>
__global__ __launch_bounds__(256)
void final_gather_kernel(const pgpu_small_query* __restrict__ sq, const pgpu_small_result* __restrict__ sr, uint32_t n,
                         pgpu_final_result* __restrict__ res, uint32_t* __restrict__ counts,
                         const unsigned long long* __restrict__ first, const pgpu_factor* __restrict__ ex_sout,
                         const uint8_t* __restrict__ ssteps, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pgpu_final_result r = res[i];
  if (WRITE) {
    if (r.outcome != PGPU_FACT_DONE) return;
    const unsigned long long at = first[i];
    const size_t from = 2 * (size_t)sq[i].first_exon + sr[i].first_kept;
    for (uint32_t k = 0; k < r.n_exons; ++k) {
      out_exons[at + k] = ex_sout[from + k];
      out_steps[at + k] = ssteps[from + k];
    }
    res[i].first_exon = (uint32_t)at;
    return;
  }
  if (r.outcome == FINAL_PENDING) {
    const pgpu_small_result a = sr[i];
    if (a.status != PGPU_OK) { settle(r, PGPU_FACT_HOST, 5, 1); r.refused = a.refused; }
    else {
      r.n_added = (uint16_t)a.n_added; r.n_cleaned = (uint16_t)(a.n_list - a.n_kept); r.prefix_added = a.prefix_added;
      if (a.verdict != 0) settle(r, PGPU_FACT_EMPTY, 5, a.verdict);
      else { settle(r, PGPU_FACT_DONE, 5, r.detail & 1u); r.n_exons = (uint16_t)a.n_kept; }
    }
    res[i] = r;
  }
  counts[i] = r.outcome == PGPU_FACT_DONE ? r.n_exons : 0u;
}

thread_local double t_final_ms = 0.0;

}  // namespace

hipError_t pgpu_final_drive(pgpu_ctx* ctx, pgpu_final_job& d) {
  const uint32_t n = d.n, E = d.n_exons_total;
  d.total = 0;
  if (n == 0) return hipSuccess;                       // no kernel is ever launched with an empty grid
  const size_t scan_tmp = pgpu_scan_tmp_bytes((size_t)n + 1);
  const FactLayout F = fact_layout(n, E, scan_tmp);
  const FinalLayout L = final_layout(n, E, scan_tmp);
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  pgpu_factor* const ex_tin = (pgpu_factor*)(B + L.ex_tin);
  pgpu_factor* const ex_tout = (pgpu_factor*)(B + L.ex_tout);
  pgpu_factor* const ex_sin = (pgpu_factor*)(B + L.ex_sin);
  pgpu_factor* const ex_sout = (pgpu_factor*)(B + L.ex_sout);
  pgpu_tail_query* const tq = (pgpu_tail_query*)(B + L.tq);
  pgpu_tail_result* const tr = (pgpu_tail_result*)(B + L.tr);
  pgpu_small_query* const sq = (pgpu_small_query*)(B + L.sq);
  pgpu_small_result* const sr = (pgpu_small_result*)(B + L.sr);
  pgpu_final_result* const res = (pgpu_final_result*)(B + L.res);
  uint32_t* const counts = (uint32_t*)(B + L.counts);
  unsigned long long* const first = (unsigned long long*)(B + L.first);
  const uint32_t tlen = d.ix.n;
  const dim3 grid((n + 255) / 256), blk(256);
  size_t waves = 0, cus = 0;
  DRIVE(chained_waves(n, waves, cus));

  DRIVE(drive_record(d.ev, 0, st));
  hipLaunchKernelGGL(final_to_tail_kernel, grid, blk, 0, st, d.fq, d.pat_off, d.orig_off, (const pgpu_fact_result*)(d.fact_block + F.res),
                     (const pgpu_factor*)(d.fact_block + F.out_exons), n, E, d.ests_len, tlen, ex_tin, tq, res);
  DRIVE(drive_record(d.ev, 2, st));
  if (d.given_tail) {
    DRIVE(hipMemcpyAsync(tr, d.given_tail->results, n * sizeof *tr, hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(ex_tout, d.given_tail->exons, ((size_t)E + n) * sizeof(pgpu_factor), hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(B + L.tsteps, d.given_tail->steps, (size_t)E + n, hipMemcpyHostToDevice, st));
  } else (d.wide ? pgpu_tail_wide_launch : pgpu_tail_launch)(d.ix.T, tlen, d.ests, ex_tin, tq, n, waves, ex_tout, B + L.tsteps, tr, st);
  DRIVE(drive_record(d.ev, 3, st));
  hipLaunchKernelGGL(final_tail_to_small_kernel, grid, blk, 0, st, tq, tr, n, E, d.ests_len, tlen, ex_tout, B + L.tsteps, ex_sin, sq, res);
  DRIVE(drive_record(d.ev, 4, st));
  if (d.given_small) {
    DRIVE(hipMemcpyAsync(sr, d.given_small->results, n * sizeof *sr, hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(ex_sout, d.given_small->exons, 2 * ((size_t)E + n) * sizeof(pgpu_factor), hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(B + L.ssteps, d.given_small->steps, 2 * ((size_t)E + n), hipMemcpyHostToDevice, st));
  } else (d.wide ? pgpu_small_wide_launch : pgpu_small_launch)(d.ix, *d.cv, d.ests, ex_sin, sq, n, d.min_intron_length, waves, ex_sout, B + L.ssteps, sr, st);
  DRIVE(drive_record(d.ev, 5, st));
  hipLaunchKernelGGL(final_gather_kernel<false>, grid, blk, 0, st, sq, sr, n, res, counts, (const unsigned long long*)nullptr,
                     (const pgpu_factor*)nullptr, (const uint8_t*)nullptr, (pgpu_factor*)nullptr, (uint8_t*)nullptr);
  DRIVE(drive_scan(counts, first, n, B + L.scan_tmp, st));
  hipLaunchKernelGGL(final_gather_kernel<true>, grid, blk, 0, st, sq, sr, n, res, (uint32_t*)nullptr, first, ex_sout, B + L.ssteps,
                     (pgpu_factor*)(B + L.out_exons), B + L.out_steps);
  DRIVE(drive_record(d.ev, 1, st));
  return drive_total(ctx, first, n, &d.total);
}

extern "C" double pgpu_index_final_factorizations_kernel_ms(void) { return t_final_ms; }

// the entry in its two forms: `wide` is pgpu_final_job's
static int final_factorizations_call(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_factor* exons,
                                     size_t n_exons_total, const pgpu_final_query* q, size_t n, const pgpu_fact_params* params,
                                     const pgpu_small_params* small_params, pgpu_final_result* out, pgpu_factor* out_exons,
                                     uint8_t* out_steps, size_t cap, size_t* n_out, const bool wide) {
  t_final_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_final_query) == 32 && sizeof(pgpu_final_result) == 32 && sizeof(pgpu_small_params) == 8, "ABI layout");
  if (!ctx || !idx || !params || !small_params || !n_out || (n && (!q || !out)) || (ests_len && !ests) ||
      (n_exons_total && !exons) || (cap && (!out_exons || !out_steps)))
    return PGPU_EINVAL;
  if (n > 0x7fffffffull || n_exons_total > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, FACT_TOO_MANY);
  if (!fact_params_ok(*params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, FACT_BAD_PARAMS);
  if (!small_params_ok(small_params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, SMALL_BAD_PARAMS);
  NamedExons named;
  named.p = (uint8_t*)calloc(n_exons_total ? n_exons_total : 1, 1);
  const std::unique_ptr<pgpu_fact_query, void (*)(void*)> fact_queries((pgpu_fact_query*)calloc(n ? n : 1, sizeof(pgpu_fact_query)), free);
  pgpu_fact_query* const fq = fact_queries.get();      // what the first driver takes of the queries
  if (!named.p || !fq) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "no memory for the table of the exons the queries name");
  if (!final_queries_ok(q, n, ests_len, n_exons_total, named.p, fq))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad final query (a range past its buffer, an empty EST, reserved != 0, or an exon two "
                                           "queries share)");
  *n_out = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  ClassView cv;
  if (const int rc = pgpu_class_view_get(ctx, idx, &cv)) return rc;
  QueryCall call(ctx, "final factorizations");
  // the one device block: [ests + 64 | final queries | factorization queries | the first driver's block | the second one's];
  // the workspace of clean and refine in a second one, once it is sized
  const size_t scan_tmp = pgpu_scan_tmp_bytes(n + 1);
  const FactLayout F = fact_layout(n, n_exons_total, scan_tmp);
  const FinalLayout L = final_layout(n, n_exons_total, scan_tmp);
  BlockCarver c{up256(ests_len + 64)};
  const size_t o_q = c.take(n * sizeof *q), o_fq = c.take(n * sizeof *fq), o_fact = c.take(F.total), o_final = c.take(L.total);
  TRY_HIP(hipMalloc((void**)&call.d, c.at));
  TRY_HIP(call.timing_events(7));                      // the eight of pgpu_fact_job, then the six of pgpu_final_job
  if (ests_len) TRY_HIP(hipMemcpyAsync(call.d, ests, ests_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_q, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_fq, fq, n * sizeof *fq, hipMemcpyHostToDevice, call.st));
  pgpu_fact_job job;
  TRY_HIP(pgpu_fact_index_job(call, idx, o_fq, o_fact, exons, n_exons_total, n, job));
  TRY_HIP(pgpu_fact_drive(ctx, job, *params));
  if (job.undersized) return pgpu_clean_undersized(ctx, "final factorizations");
  pgpu_final_job fin;
  fin.ix = pgpu_index_small_view(idx); fin.cv = &cv;
  fin.ests = call.d; fin.ests_len = ests_len;
  fin.fq = (const pgpu_final_query*)(call.d + o_q); fin.pat_off = nullptr; fin.orig_off = nullptr;
  fin.n = (uint32_t)n; fin.n_exons_total = (uint32_t)n_exons_total; fin.min_intron_length = small_params->min_intron_length;
  fin.fact_block = job.block; fin.block = call.d + o_final; fin.wide = wide;
  for (int k = 0; k < 6; ++k) fin.ev[k] = call.ev[8 + k];
  TRY_HIP(pgpu_final_drive(ctx, fin));
  *n_out = (size_t)fin.total;
  if (fin.total > cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  TRY_HIP(drive_download(fin.block, L, n * sizeof *out, fin.total, out, out_exons, out_steps, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  if (call.ev[0]) { float ms = 0.f; (void)hipEventElapsedTime(&ms, call.ev[0], call.ev[9]); t_final_ms = ms; }
  return PGPU_OK;
}

extern "C" int pgpu_index_final_factorizations(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                               const pgpu_factor* exons, size_t n_exons_total, const pgpu_final_query* q, size_t n,
                                               const pgpu_fact_params* params, const pgpu_small_params* small_params,
                                               pgpu_final_result* out, pgpu_factor* out_exons, uint8_t* out_steps, size_t cap,
                                               size_t* n_out) {
  return final_factorizations_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, params, small_params, out, out_exons,
                                   out_steps, cap, n_out, false);
}

extern "C" int pgpu_index_final_factorizations_wide(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                                    const pgpu_factor* exons, size_t n_exons_total, const pgpu_final_query* q,
                                                    size_t n, const pgpu_fact_params* params, const pgpu_small_params* small_params,
                                                    pgpu_final_result* out, pgpu_factor* out_exons, uint8_t* out_steps, size_t cap,
                                                    size_t* n_out) {
  return final_factorizations_call(ctx, idx, ests, ests_len, exons, n_exons_total, q, n, params, small_params, out, out_exons,
                                   out_steps, cap, n_out, true);
}

// ---- the hand-off kernels alone, for the tests (declared nowhere in include/pintron_gpu.h) ----------------------------
// The second driver over stage results the caller has made: `fres` and `fexons` (n_exons_total entries) stand for the
// first driver's answer, `tail` and `small` for what the two stage kernels would have written (arrays of n_exons_total + n
// and twice as many entries, in the block's layout); no stage kernel runs and no EST byte is read.  What no input brings
// through clean, gaps and refine -- 65 exons, a coordinate equal to a length, a disordered list, every refusal code -- reaches
// the three kernels this way.  Structure is checked so that no kernel leaves its arrays: DONE ranges ascending and disjoint
// inside fexons, and a kept run of small inside the two slots per exon of its EST.  tlen, ests_len: what the validators
// compare with.  Out: tq, sq (n each), ex_sin (n_exons_total + n), res, and the compact answer (2 * n_exons_total entries).
extern "C" int pgpu_final_handoffs_probe(pgpu_ctx* ctx, uint32_t tlen, size_t ests_len, const pgpu_final_query* q, size_t n,
                                         const pgpu_fact_result* fres, const pgpu_factor* fexons, size_t n_exons_total,
                                         const pgpu_tail_result* tail_res, const pgpu_factor* tail_exons, const uint8_t* tail_steps,
                                         const pgpu_small_result* small_res, const pgpu_factor* small_exons, const uint8_t* small_steps,
                                         pgpu_tail_query* tq, pgpu_small_query* sq, pgpu_factor* ex_sin, pgpu_final_result* out,
                                         pgpu_factor* out_exons, uint8_t* out_steps, size_t* n_out) {
  if (!ctx || !q || !fres || !fexons || !tail_res || !tail_exons || !tail_steps || !small_res || !small_exons || !small_steps || !tq ||
      !sq || !ex_sin || !out || !out_exons || !out_steps || !n_out || n == 0 || n_exons_total == 0 || n > 0xffffffu ||
      n_exons_total > 0xffffffu)
    return PGPU_EINVAL;
  size_t next = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool done = fres[i].outcome == PGPU_FACT_DONE;
    if (done && (fres[i].first_exon < next || fres[i].n_exons == 0 || fres[i].first_exon + (size_t)fres[i].n_exons > n_exons_total))
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "probe: DONE ranges must ascend inside the exons");
    if (done) next = fres[i].first_exon + (size_t)fres[i].n_exons;
    if ((size_t)small_res[i].first_kept + small_res[i].n_kept > 2 * (size_t)(done ? fres[i].n_exons : 1))
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "probe: a kept run outside its list");
  }
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, nullptr);
  const size_t scan_tmp = pgpu_scan_tmp_bytes(n + 1);
  const FactLayout F = fact_layout(n, n_exons_total, scan_tmp);
  const FinalLayout L = final_layout(n, n_exons_total, scan_tmp);
  const size_t o_fact = up256(n * sizeof *q), o_final = o_fact + F.total;
  TRY_HIP(hipMalloc((void**)&call.d, o_final + L.total));
  TRY_HIP(hipMemcpyAsync(call.d, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_fact + F.res, fres, n * sizeof *fres, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_fact + F.out_exons, fexons, n_exons_total * sizeof(pgpu_factor), hipMemcpyHostToDevice, call.st));
  const pgpu_final_job::Given gt = { tail_res, tail_exons, tail_steps }, gs = { small_res, small_exons, small_steps };
  pgpu_final_job fin;
  fin.ix = LcfIndexView{}; fin.ix.n = tlen; fin.cv = nullptr;
  fin.ests = nullptr; fin.ests_len = ests_len;
  fin.fq = (const pgpu_final_query*)call.d; fin.pat_off = nullptr; fin.orig_off = nullptr;
  fin.fact_block = call.d + o_fact;
  fin.n = (uint32_t)n; fin.n_exons_total = (uint32_t)n_exons_total; fin.min_intron_length = 0;
  fin.block = call.d + o_final;
  for (auto& e : fin.ev) e = nullptr;
  fin.given_tail = &gt; fin.given_small = &gs;
  TRY_HIP(pgpu_final_drive(ctx, fin));
  *n_out = (size_t)fin.total;
  TRY_HIP(hipMemcpyAsync(tq, fin.block + L.tq, n * sizeof *tq, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(hipMemcpyAsync(sq, fin.block + L.sq, n * sizeof *sq, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(hipMemcpyAsync(ex_sin, fin.block + L.ex_sin, (n_exons_total + n) * sizeof(pgpu_factor), hipMemcpyDeviceToHost, call.st));
  TRY_HIP(drive_download(fin.block, L, n * sizeof *out, fin.total, out, out_exons, out_steps, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  return PGPU_OK;
}
