// The candidate factorization of a MEG that is one path, from its record.  Semantics: include/pintron_gpu.h
// (pgpu_pairing_plan_run_candidates, pgpu_index_candidates): the path test of the host's chain_embedding, update_embedding
// (src/est-factorizations.c:765-917) folded over the path from the sink backwards, and the exons of
// get_factorizations_from_embeddings (:1292-1356).
//
//   cand_kernel<false>   one thread per record, as meg_build_kernel / meg_emit_kernel: the fold is a serial chain of at most
//                        62 steps over the 12-byte vertices of one record, and its cut scans are a handful of cuts wide.
//                        Writes the result (kind, work, n_exons, n_pairs) and the exon count for the scan.
//   cand_kernel<true>    behind pgpu_exclusive_scan_u32: the fold again for the records of kind ONE, storing the exons back
//                        to front into the compact array and first_exon into the result.
// The embedding is never stored: a step fixes the length of the node it adds and the start of the head it trims, and
// nothing older changes again, so the state is the head, the ends of the exon it lies in, and three counters.  The path is
// not stored either: the vertex in front of one is found in the record's target bytes (a path has one edge per vertex but
// the sink, so edge e belongs to vertex e, or e + 1 behind the sink).  No LDS, no stack frame.
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_stage_drive.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_cand.h"

namespace {

struct RecView {
  const int32_t* vt;        // n_vertices x (p, t, l)
  const uint16_t* first;    // CSR
  const uint8_t* tgt;
  uint32_t nv;
};

// the path test: the index of the sink when the graph is one path from vertex 0 through every vertex, else -1
__device__ int path_sink(const RecView& R) {
  if (R.nv < 2 || R.nv > PGPU_MEG_MAX_VERTICES) return -1;
  if (R.vt[0] != CAND_SOURCE_P) return -1;
  unsigned long long seen = 0;
  uint32_t k = 0, n = 0;
  for (;;) {
    if (seen >> k & 1ull) return -1;
    seen |= 1ull << k; ++n;
    const uint32_t f0 = R.first[k], deg = (uint32_t)R.first[k + 1] - f0;
    if (deg == 0) break;
    if (deg != 1) return -1;
    k = R.tgt[f0];
    if (k >= R.nv) return -1;
  }
  if (n != R.nv || R.vt[3 * k] != CAND_SINK_P) return -1;
  return (int)k;
}

// the vertex whose only edge leads to k, on a graph path_sink accepted (every vertex but the sink has one edge; k is not the
// source).  The records of the MEG stage number the vertices along the EST, so the one in front is tried first.
__device__ uint32_t path_pred(const RecView& R, uint32_t sink, uint32_t k) {
  uint32_t j = k - 1;
  if (j != sink && R.tgt[R.first[j]] == k) return j;
  for (j = 0; j + 1 < R.nv; ++j)
    if (j != sink && R.tgt[R.first[j]] == k) break;
  return j;
}

// The fold and the exons.  WRITE: the exons go to ex_last, ex_last - 1, ... (ex_last = the candidate's last slot).
// Returns the kind; work, n_exons and n_pairs as the header defines them.
template <bool WRITE>
__device__ uint32_t fold(const RecView& R, uint32_t sink, const uint8_t* __restrict__ T, uint32_t tlen, int L, int min_intron,
                         pgpu_factor* ex_last, uint32_t& work, uint32_t& n_exons, uint32_t& n_pairs) {
  const int fl = 2 * L;
  work = R.nv; n_exons = 0; n_pairs = 0;
  int head_p = R.vt[3 * sink], head_t = R.vt[3 * sink + 1], head_l = R.vt[3 * sink + 2];
  int end_e = 0, end_g = 0;                                 // the ends of the exon the head lies in
  uint32_t k = sink;
  for (uint32_t step = 1; step < R.nv; ++step) {
    k = path_pred(R, sink, k);
    const int node_p = R.vt[3 * k], node_t = R.vt[3 * k + 1], node_len = R.vt[3 * k + 2];
    if (head_p == CAND_SINK_P) {
      if (node_p < 0) return PGPU_CAND_REFUSED;
      head_p = node_p; head_t = node_t; head_l = node_len;
      end_e = node_p + node_len - 1; end_g = node_t + node_len - 1;
      n_pairs = 1; n_exons = 0;
      ++work;
      continue;
    }
    if (node_p < 0) { ++work; continue; }                   // the source copies the embedding
    const int small_delta = (head_p + head_l) - node_p;
    const int big_delta = (head_t + head_l) - node_t;
    if (!(small_delta >= fl && big_delta >= fl)) return PGPU_CAND_REFUSED;
    if (!(small_delta - (node_len + head_l) <= fl)) return PGPU_CAND_REFUSED;
    if (!((long long)small_delta - big_delta <= fl)) return PGPU_CAND_REFUSED;
    int nh_l, nh_p, nh_t, node_l;
    if (small_delta >= node_len + head_l && big_delta >= node_len + head_l) {
      nh_p = head_p; nh_t = head_t; nh_l = head_l; node_l = node_len;
    } else {
      const int ref_delta = small_delta < big_delta ? small_delta : big_delta;
      int len_node = ref_delta / 2;
      int len_head = ref_delta - len_node;
      if (len_node > node_len) { len_node = node_len; len_head = ref_delta - len_node; }
      else if (len_head > head_l) { len_head = head_l; len_node = ref_delta - len_head; }
      nh_l = len_head;
      nh_p = head_p + head_l - nh_l;
      nh_t = head_t + head_l - nh_l;
      node_l = len_node;
    }
    const bool overlap_on_p = small_delta < node_len + head_l;
    const int gap_on_p = nh_p - node_p - node_l - 1;
    const int gap_on_t = nh_t - node_t - node_l - 1;
    const int intron_len = gap_on_t - (gap_on_p > 0 ? gap_on_p : 0);
    const bool intron_on_t = intron_len >= 0 && (min_intron == 0 || intron_len >= min_intron);
    if (overlap_on_p && intron_on_t) {                      // the best cut by Burset frequency; the last of equals
      int best_freq = -1, best_cut = 0;
      const int lo = node_p + L > head_p ? node_p + L : head_p;
      const int hi = head_p + head_l - L < node_p + node_len ? head_p + head_l - L : node_p + node_len;
      for (int cut = lo; cut <= hi; ++cut) {
        const int f = burset_adaptor(T, tlen, (uint32_t)(cut - node_p + node_t), (uint32_t)(cut - head_p + head_t));
        if (f >= best_freq) { best_freq = f; best_cut = cut; }
      }
      const int dH = best_cut - head_p;
      nh_l = head_l - dH; nh_p = head_p + dH; nh_t = head_t + dH;
      node_l = node_len - (node_p + node_len - best_cut);
    }
    if (!(gap_on_t <= fl || intron_on_t)) return PGPU_CAND_REFUSED;
    // the trimmed head is final from here on: does an exon begin with it (:1292-1356)?
    if (nh_t - (node_t + node_l - 1) - 1 > fl) {
      if (WRITE) { pgpu_factor f; f.EST_start = nh_p; f.EST_end = end_e; f.GEN_start = nh_t; f.GEN_end = end_g; *(ex_last - n_exons) = f; }
      ++n_exons;
      end_e = node_p + node_l - 1; end_g = node_t + node_l - 1;
    }
    head_p = node_p; head_t = node_t; head_l = node_l;
    ++n_pairs; ++work;
  }
  if (head_p == CAND_SINK_P) return PGPU_CAND_REFUSED;      // (unreachable: the vertex in front of the sink settles it)
  if (WRITE) { pgpu_factor f; f.EST_start = head_p; f.EST_end = end_e; f.GEN_start = head_t; f.GEN_end = end_g; *(ex_last - n_exons) = f; }
  ++n_exons;
  return PGPU_CAND_ONE;
}

template <bool WRITE>
__global__ __launch_bounds__(64)
void cand_kernel(const uint8_t* __restrict__ recs, const unsigned long long* __restrict__ rec_first, uint32_t n,
                 const uint8_t* __restrict__ T, uint32_t tlen, pgpu_cand_params prm, pgpu_cand_result* __restrict__ res,
                 uint32_t* __restrict__ counts, const unsigned long long* __restrict__ first_exon, pgpu_factor* __restrict__ exons) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* rec = recs + rec_first[i];
  const uint32_t* head = (const uint32_t*)rec;
  RecView R;
  R.nv = head[0];
  R.vt = (const int32_t*)(rec + 16);
  R.first = (const uint16_t*)(rec + 16 + 12 * (size_t)R.nv);
  R.tgt = rec + 16 + 12 * (size_t)R.nv + 2 * ((size_t)R.nv + 1);
  if (WRITE) {
    const pgpu_cand_result r = res[i];
    if (r.kind != PGPU_CAND_ONE) return;
    const unsigned long long at = first_exon[i];
    res[i].first_exon = (uint32_t)at;
    int sink = 0;                                            // the sink is the vertex without an out-edge
    while (R.first[sink + 1] != R.first[sink]) ++sink;
    uint32_t work, ne, np;
    fold<true>(R, (uint32_t)sink, T, tlen, (int)prm.min_factor_len, prm.min_intron_length, exons + at + r.n_exons - 1, work, ne, np);
    return;
  }
  pgpu_cand_result r;
  r.kind = PGPU_CAND_NONE; r.work = 0; r.first_exon = 0; r.n_exons = 0; r.n_pairs = 0;
  if (!(head[2] & (PGPU_MEG_UNAVAILABLE | PGPU_MEG_TOO_COMPLEX))) {
    const int sink = path_sink(R);
    r.kind = PGPU_CAND_NOT_PATH;
    if (sink >= 0) {
      uint32_t work, ne, np;
      r.kind = fold<false>(R, (uint32_t)sink, T, tlen, (int)prm.min_factor_len, prm.min_intron_length, nullptr, work, ne, np);
      r.work = work;
      if (r.kind == PGPU_CAND_ONE) { r.n_exons = (uint16_t)ne; r.n_pairs = (uint16_t)np; }
    }
  }
  res[i] = r;
  counts[i] = r.n_exons;
}

thread_local double t_cand_ms = 0.0;

}  // namespace

void pgpu_cand_launch_count(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                            const pgpu_cand_params* prm, pgpu_cand_result* res, uint32_t* counts, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(cand_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, st, recs, rec_first, n, T, tlen, *prm, res, counts,
                     (const unsigned long long*)nullptr, (pgpu_factor*)nullptr);
}

void pgpu_cand_launch_write(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                            const pgpu_cand_params* prm, pgpu_cand_result* res, const unsigned long long* first_exon,
                            pgpu_factor* exons, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(cand_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, st, recs, rec_first, n, T, tlen, *prm, res,
                     (uint32_t*)nullptr, first_exon, exons);
}

extern "C" double pgpu_index_candidates_kernel_ms(void) { return t_cand_ms; }

extern "C" int pgpu_index_candidates(pgpu_ctx* ctx, const pgpu_index* idx, const void* records, size_t records_len,
                                     const uint64_t* rec_first, size_t n, const pgpu_cand_params* params,
                                     pgpu_cand_result* out, pgpu_factor* exons, size_t exons_cap, size_t* n_exons) {
  t_cand_ms = 0.0;       // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_cand_params) == 8 && sizeof(pgpu_cand_result) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  if (!ctx || !idx || !params || !n_exons || (n && (!rec_first || !out)) || (records_len && !records) || (exons_cap && !exons))
    return PGPU_EINVAL;
  if (n > 0x7fffffffull) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 records in one call");
  if (!cand_params_ok(*params)) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad candidate parameters (min_factor_len 0 or above 2^24)");
  if (!cand_records_ok(records, records_len, rec_first, n, pgpu_index_length(idx)))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad MEG record (offsets not ascending, past the buffer or not at a multiple of 4, a record "
                                           "shorter than its counts need, more than 64 vertices, CSR offsets out of order or past "
                                           "n_edges, a target that is no vertex, or a vertex outside what it indexes)");
  *n_exons = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "candidates");
  // the one device block: [records | offsets | results | counts (n + 1) | first_exon (n + 1) | scan workspace]; the exons
  // in a second one, sized by the scan
  const size_t rec_bytes = (size_t)rec_first[n];
  BlockCarver c{up256(rec_bytes + 4)};
  const size_t o_first = c.take((n + 1) * sizeof(uint64_t)), o_res = c.take(n * sizeof(pgpu_cand_result)),
               o_cnt = c.take((n + 1) * sizeof(uint32_t)), o_off = c.take((n + 1) * sizeof(uint64_t)),
               o_tmp = c.take(pgpu_scan_tmp_bytes(n + 1));
  TRY_HIP(hipMalloc((void**)&call.d, c.at));
  TRY_HIP(call.timing_events(2));
  if (rec_bytes) TRY_HIP(hipMemcpyAsync(call.d, records, rec_bytes, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_first, rec_first, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
  const uint8_t* const T = pgpu_index_genomic(idx);
  const uint32_t tlen = (uint32_t)pgpu_index_length(idx);
  pgpu_cand_result* const d_res = (pgpu_cand_result*)(call.d + o_res);
  uint32_t* const d_cnt = (uint32_t*)(call.d + o_cnt);
  unsigned long long* const d_off = (unsigned long long*)(call.d + o_off);
  const unsigned long long* const d_first = (const unsigned long long*)(call.d + o_first);
  TRY_HIP(call.record(0));
  pgpu_cand_launch_count(call.d, d_first, (uint32_t)n, T, tlen, params, d_res, d_cnt, call.st);
  TRY_HIP(drive_scan(d_cnt, d_off, n, call.d + o_tmp, call.st));
  TRY_HIP(call.record(1));
  unsigned long long total_exons = 0;
  TRY_HIP(drive_total(ctx, d_off, n, &total_exons));
  *n_exons = (size_t)total_exons;
  if (total_exons > exons_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  TRY_HIP(hipMalloc((void**)&call.d2, total_exons ? (size_t)total_exons * sizeof(pgpu_factor) : 16));
  TRY_HIP(call.record(2));
  pgpu_cand_launch_write(call.d, d_first, (uint32_t)n, T, tlen, params, d_res, d_off, (pgpu_factor*)call.d2, call.st);
  TRY_HIP(call.record(3));
  TRY_HIP(hipMemcpyAsync(out, d_res, n * sizeof(pgpu_cand_result), hipMemcpyDeviceToHost, call.st));
  if (total_exons) TRY_HIP(hipMemcpyAsync(exons, call.d2, (size_t)total_exons * sizeof(pgpu_factor), hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  double a = 0.0, b = 0.0;
  call.elapsed_ms(0, &a);
  call.elapsed_ms(1, &b);
  t_cand_ms = a + b;
  return PGPU_OK;
}
