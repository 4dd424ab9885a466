// The unit stage: from the finals of the patterns (pgpu_final.hip) to est-fact's answer per input EST -- one verdict per
// unit (an EST with its reverse-complement sibling) and, for an ALIGNED one, the bytes of its group in the packed records.
// Semantics: include/pintron_gpu.h (pgpu_unit_records, pgpu_pairing_plan_run_units).
//
// One thread per unit, twice around pgpu_exclusive_scan_u32, in the shape of final_gather_kernel:
//
//   unit_kernel<false>   the verdict of the forward pattern, of the sibling when the forward one has no factorization, the
//                        unit's result and the bytes of its group for the scan;
//   unit_kernel<true>    the group of every ALIGNED unit at its offset, compact, in unit order.
//
// A thread reads a query of 16 bytes, one or two results of 32, the exons of the patterns it judges (16-byte loads) and, for
// a pattern that is no path, twelve bytes of its MEG record's header; it writes its group in 32-bit words, every offset a
// multiple of 4.  No LDS, no per-thread array, no stack frame, no atomic: a pattern belongs to one unit and a group to one
// thread.  The one host wait of the drive is its last statement.
#include <stdlib.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_stage_drive.h"
#include "pgpu_unit.h"

namespace {

// what a pattern says: the numbering is the unit verdicts' (PGPU_UNIT_HOST / UNALIGNED / ALIGNED)
constexpr uint32_t PAT_HOST = PGPU_UNIT_HOST, PAT_NONE = PGPU_UNIT_UNALIGNED, PAT_ALIGNED = PGPU_UNIT_ALIGNED;
constexpr int64_t UB_VERY_SMALL_EXON = 2;      // _UB_VERY_SMALL_EXON_LENGTH_ (src/factorization-refinement.c:97)

// where the empty-graph bit of a pattern is read: a byte per pattern (may be null: none is empty), or the MEG records
struct UnitGraphs { const uint8_t* empty; const uint8_t* recs; const unsigned long long* rec_first; };

__device__ __forceinline__ bool graph_is_empty(const UnitGraphs& g, uint32_t p) {
  if (g.recs) {
    const unsigned long long at = g.rec_first[p];
    if (g.rec_first[p + 1] - at < 16) return false;
    const uint32_t* h = (const uint32_t*)(g.recs + at);      // records lie at multiples of 4: n_vertices, n_edges, flags
    return h[0] == 2u && h[1] == 0u && h[2] == 0u;
  }
  return g.empty && g.empty[p] != 0;
}

__device__ __forceinline__ int4 exon_at(const pgpu_factor* __restrict__ exons, size_t k) { return ((const int4*)exons)[k]; }

__device__ __forceinline__ uint32_t pattern_verdict(const pgpu_final_result& r, const pgpu_factor* __restrict__ exons,
                                                    uint32_t n_exons_total, const UnitGraphs& g, uint32_t p, uint32_t& reason) {
  reason = 0;
  if (r.outcome == PGPU_FACT_DONE) {
    // (a guard: the validator of the form without a plan and the final driver hand no such range in)
    if (r.n_exons == 0 || r.n_exons > UNIT_MAX_EXONS || r.first_exon > n_exons_total || r.n_exons > n_exons_total - r.first_exon)
      return PAT_HOST;
    for (uint32_t k = 0; k < r.n_exons; ++k) {
      const int4 e = exon_at(exons, (size_t)r.first_exon + k);
      if ((int64_t)e.y + 1 - (int64_t)e.x <= UB_VERY_SMALL_EXON) { reason = 1; return PAT_NONE; }
    }
    return PAT_ALIGNED;
  }
  if (r.outcome == PGPU_FACT_EMPTY) return PAT_NONE;
  if (r.outcome == PGPU_FACT_HOST && r.stage == 0 && r.detail == PGPU_CAND_NOT_PATH && graph_is_empty(g, p)) { reason = 2; return PAT_NONE; }
  return PAT_HOST;
}

template <bool WRITE>
__global__ __launch_bounds__(256)
void unit_kernel(const pgpu_unit_query* __restrict__ uq, uint32_t n, const pgpu_final_result* __restrict__ res,
                 const pgpu_factor* __restrict__ exons, uint32_t n_exons_total, const UnitGraphs g, const uint32_t pref_N,
                 const uint32_t retain, pgpu_unit_result* __restrict__ out, uint32_t* __restrict__ counts,
                 const unsigned long long* __restrict__ first, uint32_t* __restrict__ blob) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgpu_unit_query q = uq[i];
  if (WRITE) {
    const pgpu_unit_result o = out[i];
    if (o.verdict != PGPU_UNIT_ALIGNED) return;
    const unsigned long long at = first[i];
    out[i].first_byte = at;
    uint32_t* __restrict__ w = blob + (at >> 2);
    w[0] = q.est_index; w[1] = o.n_factorizations;
    if (!o.n_factorizations) return;
    const pgpu_final_result r = res[o.pattern];
    const uint32_t n_written = (o.n_bytes - 12u) >> 4, lo = retain ? 0u : 1u;
    w[2] = (retain ? (uint32_t)r.polyA | (uint32_t)r.polyadenil << 8 : 0u) | n_written << 16;
    for (uint32_t k = 0; k < n_written; ++k) {
      const int4 e = exon_at(exons, (size_t)r.first_exon + lo + k);
      w[3 + 4 * k] = (uint32_t)e.x + 1u; w[4 + 4 * k] = (uint32_t)e.y + 1u;
      w[5 + 4 * k] = pref_N + (uint32_t)e.z + 1u; w[6 + 4 * k] = pref_N + (uint32_t)e.w + 1u;
    }
    return;
  }
  uint32_t strand = 0, pat = q.fwd, reason = 0;
  pgpu_final_result r = res[pat];
  uint32_t v = pattern_verdict(r, exons, n_exons_total, g, pat, reason);
  if (v == PAT_NONE && q.rev != PGPU_UNIT_NO_SIBLING) {
    strand = 1; pat = q.rev;
    r = res[pat];
    v = pattern_verdict(r, exons, n_exons_total, g, pat, reason);
  }
  pgpu_unit_result o;
  o.verdict = (uint8_t)v; o.strand = (uint8_t)strand; o.reason = (uint8_t)reason; o.n_factorizations = 0;
  o.pattern = pat; o.first_byte = 0; o.n_bytes = 0; o.reserved = 0;
  if (v == PAT_ALIGNED) {
    const uint32_t ne = r.n_exons, suffix = (q.flags >> strand) & 1u;
    // write_multifasta_output (src/io-multifasta.c:187-241): l_index, r_index and the test in front of them
    const bool written = retain || ne > 2 || (ne == 2 && suffix);
    const uint32_t lo = retain ? 0u : 1u, hi = retain || suffix ? ne : ne - 1u;
    o.n_factorizations = written ? 1 : 0;
    o.n_bytes = 8u + (written ? 4u + 16u * (hi - lo) : 0u);
  }
  out[i] = o;
  counts[i] = o.n_bytes;
}

thread_local double t_unit_ms = 0.0;

}  // namespace

hipError_t pgpu_unit_drive(pgpu_ctx* ctx, pgpu_unit_job& d) {
  const uint32_t n = d.n;
  d.total = 0;
  if (n == 0) return hipSuccess;                       // no kernel is ever launched with an empty grid
  const UnitLayout L = unit_layout(n, d.n_done_exons, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  const pgpu_unit_query* const uq = (const pgpu_unit_query*)(B + L.q);
  pgpu_unit_result* const out = (pgpu_unit_result*)(B + L.out);
  uint32_t* const counts = (uint32_t*)(B + L.counts);
  unsigned long long* const first = (unsigned long long*)(B + L.first);
  const UnitGraphs g = { d.empty, d.recs, d.rec_first };
  const uint32_t pref_N = (uint32_t)d.params.pref_N_length, retain = d.params.retain_externals;
  const dim3 grid((n + 255) / 256), blk(256);
  DRIVE(drive_record(d.ev, 0, st));
  hipLaunchKernelGGL(unit_kernel<false>, grid, blk, 0, st, uq, n, d.res, d.exons, d.n_exons_total, g, pref_N, retain, out, counts,
                     (const unsigned long long*)nullptr, (uint32_t*)nullptr);
  DRIVE(drive_scan(counts, first, n, B + L.scan_tmp, st));
  hipLaunchKernelGGL(unit_kernel<true>, grid, blk, 0, st, uq, n, d.res, d.exons, d.n_exons_total, g, pref_N, retain, out,
                     (uint32_t*)nullptr, first, (uint32_t*)(B + L.blob));
  DRIVE(drive_record(d.ev, 1, st));
  return drive_total(ctx, first, n, &d.total);
}

extern "C" double pgpu_unit_records_kernel_ms(void) { return t_unit_ms; }

extern "C" int pgpu_unit_records(pgpu_ctx* ctx, const pgpu_final_result* res, size_t n_pat, const pgpu_factor* exons,
                                 size_t n_exons_total, const uint8_t* empty_graph, const pgpu_unit_query* q, size_t n,
                                 const pgpu_unit_params* params, pgpu_unit_result* out, void* blob, size_t blob_cap, size_t* blob_len) {
  t_unit_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_unit_query) == 16 && sizeof(pgpu_unit_params) == 8 && sizeof(pgpu_unit_result) == 24, "ABI layout");
  if (!ctx || !params || !blob_len || (n && (!q || !out)) || (n_pat && !res) || (n_exons_total && !exons) || (blob_cap && !blob))
    return PGPU_EINVAL;
  if (n > UNIT_MAX_COUNT || n_pat > UNIT_MAX_COUNT) return pgpu_ctx_fail(ctx, PGPU_EINVAL, UNIT_TOO_MANY);
  if (const char* wrong = unit_params_wrong(*params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  if (const char* wrong = unit_finals_wrong(res, n_pat, n_exons_total)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  NamedExons named;                                    // here: which patterns a unit has named already
  named.p = (uint8_t*)calloc(n_pat ? n_pat : 1, 1);
  if (!named.p) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "no memory for the table of the patterns the units name");
  if (const char* wrong = unit_queries_wrong(q, n, n_pat, named.p)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, wrong);
  *blob_len = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "unit records");
  // the one device block: [results | exons | empty-graph bytes | the stage's block]; first_exon is 32 bits wide, so no
  // result names an exon behind the first 2^32 - 1
  if (n_exons_total > 0xffffffffull) n_exons_total = 0xffffffffull;
  const size_t n_done_exons = unit_finals_exons(res, n_pat);
  const UnitLayout L = unit_layout(n, n_done_exons, pgpu_scan_tmp_bytes(n + 1));
  const size_t o_ex = up256(n_pat * sizeof *res), o_empty = o_ex + up256(n_exons_total * sizeof *exons),
               o_unit = o_empty + up256(empty_graph ? n_pat : 0);
  TRY_HIP(hipMalloc((void**)&call.d, o_unit + L.total));
  TRY_HIP(call.timing_events(1));
  TRY_HIP(hipMemcpyAsync(call.d, res, n_pat * sizeof *res, hipMemcpyHostToDevice, call.st));
  if (n_exons_total) TRY_HIP(hipMemcpyAsync(call.d + o_ex, exons, n_exons_total * sizeof *exons, hipMemcpyHostToDevice, call.st));
  if (empty_graph) TRY_HIP(hipMemcpyAsync(call.d + o_empty, empty_graph, n_pat, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_unit + L.q, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  pgpu_unit_job job;
  job.res = (const pgpu_final_result*)call.d; job.exons = (const pgpu_factor*)(call.d + o_ex);
  job.n_exons_total = (uint32_t)n_exons_total; job.n_done_exons = n_done_exons;
  job.empty = empty_graph ? call.d + o_empty : nullptr; job.recs = nullptr; job.rec_first = nullptr;
  job.params = *params; job.n = (uint32_t)n; job.block = call.d + o_unit;
  job.ev[0] = call.ev[0]; job.ev[1] = call.ev[1];
  TRY_HIP(pgpu_unit_drive(ctx, job));
  *blob_len = (size_t)job.total;
  if (job.total > blob_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "blob too small");
  TRY_HIP(hipMemcpyAsync(out, job.block + L.out, n * sizeof *out, hipMemcpyDeviceToHost, call.st));
  if (job.total) TRY_HIP(hipMemcpyAsync(blob, job.block + L.blob, (size_t)job.total, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  call.elapsed_ms(0, &t_unit_ms);
  return PGPU_OK;
}
