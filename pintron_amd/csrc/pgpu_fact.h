// The rules of pgpu_index_factorizations on what a caller hands in (include/pintron_gpu.h), and the layout of the
// driver's device block: plain host code without a HIP call, in a header so that tests/hostcheck/fact_call_check.cpp runs
// the very code of the entry under the sanitizers.  Only structure is refused here: the values of the exons are judged
// per query on the device (pgpu_fact.hip), which reads no exon outside [0, n_exons_total + n) and no EST byte outside
// [est_off, est_off + est_len) (+ the slack of the block) of a query that passes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_layout.h"

constexpr int32_t FACT_MAX_SUFFPREF = 1 << 24;      // as suffpref_ok of pgpu_query_call.h
constexpr char FACT_TOO_MANY[] = "more than 2^31 - 1 queries or exons in one call";      // n and n_exons_total are 32 bits wide
constexpr char FACT_BAD_PARAMS[] ="bad factorization parameters (a suffpref length outside [0, 2^24])";

inline bool fact_params_ok(const pgpu_fact_params& p) {
  const int32_t v[3] = { p.suffpref_length_on_est, p.suffpref_length_for_intron, p.suffpref_length_on_gen };
  for (int k = 0; k < 3; ++k)
    if (v[k] < 0 || v[k] > FACT_MAX_SUFFPREF) return false;
  return true;
}

// `named`: n_exons_total bytes of 0 (one per exon: which query has named it).  No exon is read.
inline bool fact_queries_ok(const pgpu_fact_query* q, size_t n, size_t ests_len, size_t n_exons_total, uint8_t* named) {
  for (size_t i = 0; i < n; ++i) {
    const pgpu_fact_query& x = q[i];
    if (x.est_off > ests_len || x.est_len > ests_len - x.est_off || x.est_len == 0 || x.est_len > 0x7fffffffu || x.reserved != 0)
      return false;
    if (x.n_exons == 0) continue;                         // no candidate: first_exon is not looked at
    if (x.first_exon > n_exons_total || x.n_exons > n_exons_total - x.first_exon) return false;
    for (size_t k = x.first_exon; k < (size_t)x.first_exon + x.n_exons; ++k) {
      if (named[k]) return false;
      named[k] = 1;
    }
  }
  return true;
}

// The driver's device block for n ESTs and n_exons_total candidate exons.  Every exon array has n_exons_total + n entries:
// the placeholder of EST i is entry n_exons_total + i.  Offsets are multiples of 256; `total` bytes in all.
struct FactLayout {
  size_t ex_in, ex_clean, ex_gaps, ex_kept, ex_refined;      // exon arrays: the candidates, then what each stage wrote
  size_t marks, gsteps, rsteps;                              // one byte per exon: clean's marks, gaps' and refine's steps
  size_t cq, cr, gq, gr, rq, rr;                             // per EST: the three queries and results
  size_t res, need, counts, first, scan_tmp;                 // per EST: the outcome; 3 words; the gather's scan
  size_t out_exons, out_steps;                               // the compact answer: at most n_exons_total entries
  size_t total;
};
inline FactLayout fact_layout(size_t n, size_t n_exons_total, size_t scan_tmp_bytes) {
  const size_t ne = n_exons_total + n, exb = ne * sizeof(pgpu_factor);
  FactLayout L;
  BlockCarver c;
  L.ex_in = c.take(exb); L.ex_clean = c.take(exb); L.ex_gaps = c.take(exb); L.ex_kept = c.take(exb); L.ex_refined = c.take(exb);
  L.marks = c.take(ne); L.gsteps = c.take(ne); L.rsteps = c.take(ne);
  L.cq = c.take(n * sizeof(pgpu_clean_query)); L.cr = c.take(n * sizeof(pgpu_clean_result));
  L.gq = c.take(n * sizeof(pgpu_gaps_query)); L.gr = c.take(n * sizeof(pgpu_gaps_result));
  L.rq = c.take(n * sizeof(pgpu_chain_query)); L.rr = c.take(n * sizeof(pgpu_chain_result));
  L.res = c.take(n * sizeof(pgpu_fact_result)); L.need = c.take(16);
  L.counts = c.take((n + 1) * sizeof(uint32_t)); L.first = c.take((n + 1) * sizeof(uint64_t)); L.scan_tmp = c.take(scan_tmp_bytes);
  L.out_exons = c.take(n_exons_total * sizeof(pgpu_factor)); L.out_steps = c.take(n_exons_total);
  L.total = c.at;
  return L;
}
