// The rules of pgpu_index_final_factorizations and of pgpu_pairing_plan_create_with_originals on what a caller hands in
// (include/pintron_gpu.h), and the layout of the final driver's device block: plain host code without a HIP call, in a
// header so that tests/hostcheck/final_call_check.cpp runs the very code of the entries under the sanitizers.  Only
// structure is refused here: the values of the exons are judged per query on the device (pgpu_fact.hip, pgpu_final.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_fact.h"

// The queries of the index form: what fact_queries_ok asks of the fields a final query shares with a factorization query
// -- written to fq[0 .. n), the queries the first four stages take -- and the original sequence inside the buffer as the
// working one is.  `named` as for fact_queries_ok.  No exon is read.
inline bool final_queries_ok(const pgpu_final_query* q, size_t n, size_t ests_len, size_t n_exons_total, uint8_t* named,
                             pgpu_fact_query* fq) {
  for (size_t i = 0; i < n; ++i) {
    const pgpu_final_query& x = q[i];
    fq[i].est_off = x.est_off; fq[i].est_len = x.est_len; fq[i].first_exon = x.first_exon; fq[i].n_exons = x.n_exons;
    fq[i].reserved = x.reserved;
  }
  if (!fact_queries_ok(fq, n, ests_len, n_exons_total, named)) return false;
  for (size_t i = 0; i < n; ++i)
    if (q[i].orig_off > ests_len || q[i].est_len > ests_len - q[i].orig_off) return false;
  return true;
}

// The originals of a plan: null when they are good, else what is wrong with them.  pat_off has passed the plan's own test
// (ascending, n_pat + 1 entries).  No byte of a sequence is read.
inline const char* originals_wrong(const uint64_t* pat_off, size_t n_pat, const uint32_t* orig_pat, const uint64_t* orig_first,
                                   const char* orig_bytes, size_t n_orig) {
  if (n_orig == 0) return nullptr;
  if (!orig_pat || !orig_first) return "originals: a null pointer with n_orig > 0";
  for (size_t k = 0; k < n_orig; ++k) {
    if (orig_pat[k] >= n_pat) return "originals: a pattern index beyond the plan's patterns";
    if (k && orig_pat[k] <= orig_pat[k - 1]) return "originals: the pattern indices are not strictly ascending";
    if (orig_first[k + 1] < orig_first[k] || orig_first[k + 1] - orig_first[k] != pat_off[orig_pat[k] + 1] - pat_off[orig_pat[k]])
      return "originals: an original whose length differs from its pattern's";
  }
  if (orig_first[n_orig] > orig_first[0] && !orig_bytes) return "originals: a null pointer with n_orig > 0";
  return nullptr;
}

// The final driver's device block for n ESTs whose candidates had n_exons_total exons (the refined ones are no more).  The
// tail stage's arrays have n_exons_total + n entries, the small stage's output twice as many: the placeholder of EST i is
// entry n_exons_total + i of the inputs, and its list is at twice that in small's output.  Offsets are multiples of 256.
struct FinalLayout {
  size_t ex_tin, ex_tout, ex_sin, ex_sout;      // exon arrays: tail's input and output, small's input and output
  size_t tsteps, ssteps;                        // the two stages' step bytes
  size_t tq, tr, sq, sr;                        // per EST: the two queries and results
  size_t res, counts, first, scan_tmp;          // per EST: the outcome; the gather's scan
  size_t out_exons, out_steps;                  // the compact answer: at most 2 * n_exons_total entries
  size_t total;
};
inline FinalLayout final_layout(size_t n, size_t n_exons_total, size_t scan_tmp_bytes) {
  const size_t ne = n_exons_total + n;
  FinalLayout L;
  BlockCarver c;
  L.ex_tin = c.take(ne * sizeof(pgpu_factor)); L.ex_tout = c.take(ne * sizeof(pgpu_factor));
  L.ex_sin = c.take(ne * sizeof(pgpu_factor)); L.ex_sout = c.take(2 * ne * sizeof(pgpu_factor));
  L.tsteps = c.take(ne); L.ssteps = c.take(2 * ne);
  L.tq = c.take(n * sizeof(pgpu_tail_query)); L.tr = c.take(n * sizeof(pgpu_tail_result));
  L.sq = c.take(n * sizeof(pgpu_small_query)); L.sr = c.take(n * sizeof(pgpu_small_result));
  L.res = c.take(n * sizeof(pgpu_final_result));
  L.counts = c.take((n + 1) * sizeof(uint32_t)); L.first = c.take((n + 1) * sizeof(uint64_t)); L.scan_tmp = c.take(scan_tmp_bytes);
  L.out_exons = c.take(2 * n_exons_total * sizeof(pgpu_factor)); L.out_steps = c.take(2 * n_exons_total);
  L.total = c.at;
  return L;
}
