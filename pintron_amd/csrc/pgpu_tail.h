// The rules of pgpu_index_tail_chains that concern one query alone, beside the ones every chained entry checks
// (chained_queries_ok of pgpu_query_call.h, which calls this as the entry's own): plain code without a HIP call, in a
// header so that tests/hostcheck/tail_call_check.cpp runs the very code of the entry under the sanitizers, and
// __host__ __device__ so that a driver that builds such a query on the device can ask the same of it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"

#ifdef __HIPCC__
#define PGPU_TAIL_HD __host__ __device__
#else
#define PGPU_TAIL_HD
#endif

// An EST of at least one byte; the original sequence inside the buffer as the working one is; every coordinate of every
// exon an index into what it refers to: [0, est_len) on the EST, [0, glen) on the sequence.  Stricter than factor_ok, which
// lets -1 and the length pass: step 1 reads behind the last exon's ends and step 4 in front of the first one's starts, so
// an end has to be a byte of its string.  Order between the exons, or between an exon's two ends, is no rule here: step 3
// gives its verdict on it.  The number of exons is no matter either: a query beyond PGPU_TAIL_MAX_EXONS is refused on the
// device, and its input has to be good all the same.
PGPU_TAIL_HD static inline bool tail_query_ok(const pgpu_tail_query& x, const pgpu_factor* ex, size_t ests_len, size_t glen) {
  if (x.est_len == 0) return false;
  if (x.orig_off > ests_len || x.est_len > ests_len - x.orig_off) return false;
  for (uint32_t k = 0; k < x.n_exons; ++k) {
    const pgpu_factor& f = ex[k];
    if (f.EST_start < 0 || f.EST_end < 0 || f.GEN_start < 0 || f.GEN_end < 0) return false;
    if ((uint32_t)f.EST_start >= x.est_len || (uint32_t)f.EST_end >= x.est_len) return false;
    if ((size_t)f.GEN_start >= glen || (size_t)f.GEN_end >= glen) return false;
  }
  return true;
}
