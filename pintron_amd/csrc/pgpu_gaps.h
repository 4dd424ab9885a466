// The rules of pgpu_index_gap_chains that concern one query alone, beside the ones every chained entry checks
// (chained_queries_ok of pgpu_query_call.h, which calls this as the entry's own): plain host code without a HIP call, in a
// header so that tests/hostcheck/gaps_call_check.cpp runs the very code of the entry under the sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/pintron_gpu.h"

// (the factorization driver of pgpu_fact.hip asks the same of a query it builds on the device)
#ifdef __HIPCC__
#define PGPU_GAPS_HD __host__ __device__
#else
#define PGPU_GAPS_HD
#endif

// An EST of at least one byte; every adjacent pair in order on both strings (exon[i].EST_end < exon[i + 1].EST_start,
// exon[i].GEN_end < exon[i + 1].GEN_start), and its EST gap no longer than its genomic gap (the FATAL of
// src/est-factorizations.c:1485).  With the coordinates inside [-1, length] (factor_ok) both gaps then lie inside their
// strings: [EST_end + 1, EST_start - 1] within [0, est_len - 1], and the same on the sequence.  The number of exons is
// no matter here: a query beyond PGPU_GAPS_MAX_EXONS is refused on the device, and its input has to be good all the same.
PGPU_GAPS_HD static inline bool gaps_query_ok(const pgpu_gaps_query& x, const pgpu_factor* ex) {
  if (x.est_len == 0) return false;
  for (uint32_t k = 0; k + 1 < x.n_exons; ++k) {
    const pgpu_factor& d = ex[k];
    const pgpu_factor& a = ex[k + 1];
    if (d.EST_end >= a.EST_start || d.GEN_end >= a.GEN_start) return false;
    const int64_t gap_p = (int64_t)a.EST_start - d.EST_end - 1, gap_t = (int64_t)a.GEN_start - d.GEN_end - 1;
    if (gap_p > gap_t) return false;
  }
  return true;
}
