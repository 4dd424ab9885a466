// The host side of a query on the resident index, once: what the nine entries pgpu_index_find, pgpu_index_classify,
// pgpu_index_small_exons, pgpu_index_refine_introns, pgpu_index_refine_chains, pgpu_index_clean_chains,
// pgpu_index_gap_chains, pgpu_index_tail_chains and pgpu_index_small_chains, the index forms of the four device stages
// (pgpu_index_candidates, pgpu_index_factorizations, pgpu_index_final_factorizations, pgpu_unit_records), pgpu_unit_texts, pgpu_unit_sides and
// pgpu_final_handoffs_probe share around their kernels.  An entry validates, lays out its device block, copies in, launches,
// copies out and waits, as straight-line code; the QueryCall on its stack owns what has to be given back whichever way the
// entry returns.  The five chained entries (one query = one list of exons, chained on the device) share more: the chained
// path at the end.  What the stage drivers share is in pgpu_stage_drive.h.
//
// The contract of every entry (tests/test_gpu_query_calls.py): a refused call and an empty one leave the entry's
// millisecond slot at 0; with pgpu_set_timing off the slot stays 0 and the answers are the same; a call that fails in
// HIP waits for the stream before its buffers are freed, so nothing of it outlives them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pgpu_index.h"
#include "pgpu_layout.h"

// a coordinate of a factor: -1 (unset) or an index into, or the length of, what it refers to (on the device too: the
// factorization driver of pgpu_fact.hip asks it per query)
__host__ __device__ inline bool coordinate_ok(int32_t v, size_t len) { return v >= -1 && (v < 0 || (size_t)v <= len); }
__host__ __device__ inline bool factor_ok(const pgpu_factor& f, size_t est_len, size_t gen_len) {
  return coordinate_ok(f.EST_start, est_len) && coordinate_ok(f.EST_end, est_len) && coordinate_ok(f.GEN_start, gen_len) &&
         coordinate_ok(f.GEN_end, gen_len);
}
// the three suffpref_length_* of a refine or chain query
inline bool suffpref_ok(int32_t on_est, int32_t for_intron, int32_t on_gen) {
  for (int32_t v : { on_est, for_intron, on_gen })
    if (v < 0 || v > (1 << 24)) return false;
  return true;
}

// One call: the context's stream, the device blocks (`d`; `d2` for what can be sized only after a first phase), up to seven
// pairs of events (pgpu_index_final_factorizations takes them all), and the profiler range when the entry has a name for it.
struct QueryCall {
  pgpu_ctx* const ctx;
  const hipStream_t st;
  uint8_t* d = nullptr;
  uint8_t* d2 = nullptr;
  hipEvent_t ev[14] = {nullptr};
  bool failed = false;
  const bool range;

  QueryCall(pgpu_ctx* c, const char* range_name) : ctx(c), st(pgpu_ctx_stream(c)), range(range_name != nullptr) {
    if (range) pgpu_range_push(range_name);
  }
  QueryCall(const QueryCall&) = delete;
  QueryCall& operator=(const QueryCall&) = delete;
  ~QueryCall() {
    if (failed) (void)hipStreamSynchronize(st);            // nothing of this call may outlive its buffers
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipFree(d2); (void)hipFree(d);
    if (range) pgpu_range_pop();
  }

  int fail(hipError_t e) { failed = true; return pgpu_ctx_fail(ctx, pgpu_code_of(e), hipGetErrorString(e)); }

  // `pairs` pairs of events when the context has timing on, none otherwise
  hipError_t timing_events(int pairs) {
    if (!pgpu_ctx_timing(ctx)) return hipSuccess;
    for (int i = 0; i < 2 * pairs; ++i) {
      const hipError_t e = hipEventCreate(&ev[i]);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  hipError_t record(int i) { return ev[i] ? hipEventRecord(ev[i], st) : hipSuccess; }
  // after the wait: the time between the events of pair k, into the entry's slot
  void elapsed_ms(int k, double* slot) const {
    if (!ev[2 * k]) return;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]);
    *slot = ms;
  }
};

// inside an entry whose QueryCall is named `call`
#define TRY_HIP(expr)                                   \
  do {                                                  \
    const hipError_t e_ = (expr);                       \
    if (e_ != hipSuccess) return call.fail(e_);         \
  } while (0)

// pgpu_fact.hip: the job of the two index forms over the call's one block (the ESTs at 0, the n uploaded queries at `o_fq`, the
// driver's block at `o_block`): uploads the candidate exons, takes the call's first eight events, hands ws_alloc over d2
hipError_t pgpu_fact_index_job(QueryCall& call, const pgpu_index* idx, size_t o_fq, size_t o_block, const pgpu_factor* exons,
                               size_t n_exons_total, size_t n, pgpu_fact_job& job);

// ---- The chained path: pgpu_index_refine_chains, pgpu_index_clean_chains, pgpu_index_gap_chains,
// pgpu_index_tail_chains and pgpu_index_small_chains.  Their query structs
// begin with est_off, est_len, first_exon, n_exons and reserved; the calls answer with out_exons and one byte per exon,
// parallel to `exons` (an exon no query names: a copy and byte 0; an empty call: that for every exon, without a device
// call), and with one result per query.  An entry whose lists grow (pgpu_index_small_chains) has `out_per_exon` = 2 output
// slots per input exon: a query's list is at out_per_exon * first_exon, and what no query fills is 0 instead of a copy.
// An entry keeps what the others do differently: its own rules, its workspace and its kernel.

// which exons a query has named already; calloc, for no exception may cross the C boundary
struct NamedExons { uint8_t* p = nullptr; ~NamedExons() { free(p); } };

// The rules on the common fields and on the exons a query names, then `own(query, its first exon)` for what only that
// entry checks.  No exon is read before the query's range is known to lie inside the array.  No HIP call.
template <class Query, class Own>
bool chained_queries_ok(const Query* q, size_t n, size_t ests_len, const pgpu_factor* exons, size_t n_exons_total, size_t glen,
                        uint8_t* named, Own own) {
  for (size_t i = 0; i < n; ++i) {
    const Query& x = q[i];
    if (x.est_off > ests_len || x.est_len > ests_len - x.est_off || x.est_len > 0x7fffffffu || x.reserved != 0 ||
        x.n_exons == 0 || x.first_exon > n_exons_total || x.n_exons > n_exons_total - x.first_exon)
      return false;
    for (size_t k = x.first_exon; k < (size_t)x.first_exon + x.n_exons; ++k) {
      if (named[k] || !factor_ok(exons[k], x.est_len, glen)) return false;
      named[k] = 1;
    }
    if (!own(x, exons + x.first_exon)) return false;
  }
  return true;
}

// The one device block: [ests + 64 | exons | queries | out exons | one byte per exon | results | (extra) | workspace],
// every part at a multiple of 256 (`extra_bytes`, clean's flag slot, is 0 or 256).  The sizes are the unrounded ones; the
// two output parts hold out_per_exon entries per exon.
struct ChainedLayout {
  size_t ests_len, ex_bytes, q_bytes, n_exons, r_bytes, out_per_exon;
  size_t exons, queries, out_exons, out_bytes, results, extra, ws, total;      // the ESTs are at 0
};
inline ChainedLayout chained_layout(size_t ests_len, size_t n_exons_total, size_t n, size_t query_size, size_t result_size,
                                    size_t extra_bytes, size_t ws_bytes, size_t out_per_exon = 1) {
  ChainedLayout L;
  L.out_per_exon = out_per_exon;
  L.ests_len = ests_len; L.ex_bytes = n_exons_total * sizeof(pgpu_factor); L.q_bytes = n * query_size;
  L.n_exons = n_exons_total; L.r_bytes = n * result_size;
  L.exons = up256(ests_len + 64); L.queries = L.exons + up256(L.ex_bytes); L.out_exons = L.queries + up256(L.q_bytes);
  L.out_bytes = L.out_exons + up256(out_per_exon * L.ex_bytes); L.results = L.out_bytes + up256(out_per_exon * n_exons_total);
  L.extra = L.results + up256(L.r_bytes); L.ws = L.extra + extra_bytes; L.total = L.ws + ws_bytes;
  return L;
}

// How an entry begins: a null pointer is a bare PGPU_EINVAL, then the 2^31 limit, the table, and the empty call (PGPU_OK
// with the exons copied through).  CHAINED_GO: there are queries, the call goes on.  `what`: the entry's noun in the messages.
constexpr int CHAINED_GO = 1;          // every PGPU_* code is <= 0
inline int chained_begin(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_factor* exons,
                         size_t n_exons_total, const void* q, size_t n, pgpu_factor* out_exons, uint8_t* out_bytes,
                         const void* out, const char* what, NamedExons& named, size_t out_per_exon = 1) {
  if (!ctx || !idx || (n && (!q || !out)) || (ests_len && !ests) || (n_exons_total && (!exons || !out_exons || !out_bytes)))
    return PGPU_EINVAL;
  const auto fail = [&](int code, const char* text) {
    char msg[96];
    snprintf(msg, sizeof msg, text, what);
    return pgpu_ctx_fail(ctx, code, msg);
  };
  if (n > 0x7fffffffull || n_exons_total > 0x7fffffffull) return fail(PGPU_EINVAL, "more than 2^31 - 1 %s or exons in one call");
  named.p = (uint8_t*)calloc(n_exons_total ? n_exons_total : 1, 1);
  if (!named.p) return fail(PGPU_ENOMEM, "no memory for the table of the exons the %s name");
  if (n) return CHAINED_GO;
  if (n_exons_total && out_per_exon == 1) memcpy(out_exons, exons, n_exons_total * sizeof(pgpu_factor));
  if (n_exons_total && out_per_exon != 1) memset(out_exons, 0, out_per_exon * n_exons_total * sizeof(pgpu_factor));
  if (n_exons_total) memset(out_bytes, 0, out_per_exon * n_exons_total);
  return PGPU_OK;
}

// The grid: sixteen resident waves per compute unit of the bound device (`cus`), never more waves than queries
constexpr size_t WAVES_PER_CU = 16;
inline hipError_t chained_waves(size_t n, size_t& waves, size_t& cus) {
  int dev = 0, count = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&count, hipDeviceAttributeMultiprocessorCount, dev);
  cus = (size_t)count;
  waves = n < cus * WAVES_PER_CU ? n : cus * WAVES_PER_CU;
  return e;
}

// Three copies in (a call may have no EST bytes at all), and the output seeded on the device: the exons as a copy of the
// input and their bytes as 0, which is what an exon no query names, or one of a query the kernel refuses, keeps
inline hipError_t chained_upload(const QueryCall& call, const ChainedLayout& L, const char* ests, const pgpu_factor* exons,
                                 const void* q) {
  hipError_t e = L.ests_len ? hipMemcpyAsync(call.d, ests, L.ests_len, hipMemcpyHostToDevice, call.st) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpyAsync(call.d + L.exons, exons, L.ex_bytes, hipMemcpyHostToDevice, call.st);
  if (e == hipSuccess) e = hipMemcpyAsync(call.d + L.queries, q, L.q_bytes, hipMemcpyHostToDevice, call.st);
  if (e == hipSuccess && L.out_per_exon == 1)
    e = hipMemcpyAsync(call.d + L.out_exons, call.d + L.exons, L.ex_bytes, hipMemcpyDeviceToDevice, call.st);
  if (e == hipSuccess && L.out_per_exon != 1) e = hipMemsetAsync(call.d + L.out_exons, 0, L.out_per_exon * L.ex_bytes, call.st);
  if (e == hipSuccess) e = hipMemsetAsync(call.d + L.out_bytes, 0, L.out_per_exon * L.n_exons, call.st);
  return e;
}
inline hipError_t chained_download(const QueryCall& call, const ChainedLayout& L, pgpu_factor* out_exons, uint8_t* out_bytes,
                                   void* out) {
  hipError_t e = hipMemcpyAsync(out_exons, call.d + L.out_exons, L.out_per_exon * L.ex_bytes, hipMemcpyDeviceToHost, call.st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_bytes, call.d + L.out_bytes, L.out_per_exon * L.n_exons, hipMemcpyDeviceToHost, call.st);
  if (e == hipSuccess) e = hipMemcpyAsync(out, call.d + L.results, L.r_bytes, hipMemcpyDeviceToHost, call.st);
  return e;
}
