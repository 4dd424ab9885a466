// The host side of a query on the resident index, once: what pgpu_index_find, pgpu_index_classify,
// pgpu_index_small_exons, pgpu_index_refine_introns and pgpu_index_refine_chains share around their kernels.  An
// entry validates, lays out its device block, copies in, launches, copies out and waits, as straight-line code; the
// QueryCall on its stack owns what has to be given back whichever way the entry returns.
//
// The contract of every entry (tests/test_gpu_query_calls.py): a refused call and an empty one leave the entry's
// millisecond slot at 0; with pgpu_set_timing off the slot stays 0 and the answers are the same; a call that fails in
// HIP waits for the stream before its buffers are freed, so nothing of it outlives them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pgpu_index.h"

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// what an entry returns for a HIP error
inline int pgpu_code_of(hipError_t e) { return e == hipErrorOutOfMemory ? PGPU_ENOMEM : PGPU_EDEVICE; }

// a coordinate of a factor: -1 (unset) or an index into, or the length of, what it refers to
inline bool coordinate_ok(int32_t v, size_t len) { return v >= -1 && (v < 0 || (size_t)v <= len); }
inline bool factor_ok(const pgpu_factor& f, size_t est_len, size_t gen_len) {
  return coordinate_ok(f.EST_start, est_len) && coordinate_ok(f.EST_end, est_len) && coordinate_ok(f.GEN_start, gen_len) &&
         coordinate_ok(f.GEN_end, gen_len);
}
// the three suffpref_length_* of a refine or chain query
inline bool suffpref_ok(int32_t on_est, int32_t for_intron, int32_t on_gen) {
  for (int32_t v : { on_est, for_intron, on_gen })
    if (v < 0 || v > (1 << 24)) return false;
  return true;
}

// One call: the context's stream, the device blocks (`d`; `d2` for what can be sized only after a first phase), up to two
// pairs of events, and the profiler range when the entry has a name for it.
struct QueryCall {
  pgpu_ctx* const ctx;
  const hipStream_t st;
  uint8_t* d = nullptr;
  uint8_t* d2 = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
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
