// The rules of pgpu_index_factorization_lists on what a caller hands in (include/pintron_gpu.h), and the layout of the
// driver's device block: plain host code without a HIP call, in a header so that tests/hostcheck/flists_call_check.cpp runs
// the very code of the entry under the sanitizers.  Only structure is refused here: the values of the exons are judged per
// candidate on the device (pgpu_flists.hip), which reads no candidate outside [0, n_cands_total), no exon outside
// [0, n_exons_total + n_cands_total) and no EST byte outside [est_off, est_off + est_len) (+ the slack of the block) of a
// query that passes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_layout.h"

constexpr int32_t FLIST_MAX_SETTING = 1 << 24;      // suffpref lengths, max_site_difference, max_number_of_factorizations

// every comparison is written so that a NaN fails it
inline bool flist_params_ok(const pgpu_flist_params& p) {
  const int32_t v[5] = { p.suffpref_length_on_est, p.suffpref_length_for_intron, p.suffpref_length_on_gen, p.max_site_difference,
                         p.max_number_of_factorizations };
  for (int k = 0; k < 5; ++k)
    if (v[k] < 0 || v[k] > FLIST_MAX_SETTING) return false;
  if (!(p.max_coverage_diff >= 0.0 && p.max_coverage_diff <= 1.0)) return false;
  return p.max_gaplength_diff >= -1 && p.reserved == 0;
}

// `cand_named`: n_cands_total bytes of 0 (which query has named the candidate), `exon_named`: n_exons_total bytes of 0.
// No exon is read, and no candidate before its index is known to lie inside the table.
inline bool flist_queries_ok(const pgpu_flist_query* q, size_t n, size_t ests_len, const pgpu_enum_candidate* cands,
                             size_t n_cands_total, size_t n_exons_total, uint8_t* cand_named, uint8_t* exon_named) {
  for (size_t i = 0; i < n; ++i) {
    const pgpu_flist_query& x = q[i];
    if (x.est_off > ests_len || x.est_len > ests_len - x.est_off || x.est_len == 0 || x.est_len > 0x7fffffffu || x.reserved != 0)
      return false;
    if (x.first_candidate > n_cands_total || x.n_candidates > n_cands_total - x.first_candidate) return false;
    for (size_t c = x.first_candidate; c < (size_t)x.first_candidate + x.n_candidates; ++c) {
      if (cand_named[c]) return false;
      cand_named[c] = 1;
      const pgpu_enum_candidate& k = cands[c];
      if (k.reserved != 0 || k.n_exons == 0 || k.first_exon > n_exons_total || k.n_exons > n_exons_total - k.first_exon) return false;
      for (size_t e = k.first_exon; e < (size_t)k.first_exon + k.n_exons; ++e) {
        if (exon_named[e]) return false;
        exon_named[e] = 1;
      }
    }
  }
  return true;
}

// What the entry checks without touching the device, in the entry's order.  0: the call goes on; 1 is the bare PGPU_EINVAL
// without a message.  The two tables are the caller's (calloc: no exception may cross the C boundary).
enum : int { FLIST_OK = 0, FLIST_NULL, FLIST_TOO_MANY, FLIST_PARAMS, FLIST_QUERIES };
inline int flist_call_refusal(const void* ctx, const void* idx, const void* ests, size_t ests_len, const pgpu_enum_candidate* cands,
                              size_t n_cands_total, const void* exons, size_t n_exons_total, const pgpu_flist_query* q, size_t n,
                              const pgpu_flist_params* params, const void* out, const void* facts, size_t facts_cap,
                              const void* out_exons, const void* out_steps, size_t exons_cap, const size_t* n_facts,
                              const size_t* n_exons, uint8_t* cand_named, uint8_t* exon_named) {
  if (!ctx || !idx || !params || !n_facts || !n_exons || (n && (!q || !out)) || (ests_len && !ests) || (n_cands_total && !cands) ||
      (n_exons_total && !exons) || (facts_cap && !facts) || (exons_cap && (!out_exons || !out_steps)))
    return FLIST_NULL;
  if (n > 0x7fffffffull || n_cands_total > 0x7fffffffull || n_exons_total > 0x7fffffffull) return FLIST_TOO_MANY;
  if (!flist_params_ok(*params)) return FLIST_PARAMS;
  if (!flist_queries_ok(q, n, ests_len, cands, n_cands_total, n_exons_total, cand_named, exon_named)) return FLIST_QUERIES;
  return FLIST_OK;
}

// what the driver keeps per candidate between its kernels (one writer per kernel: the candidate's thread, its record's
// thread, or its lane of the record's wave)
struct FlistSlot {
  uint32_t rec;           // the query that names the candidate; FLIST_NO_RECORD: none, or one settled at stage 0
  uint32_t first;         // the kept run of clean's out_exons: absolute index of its first exon,
  uint16_t n;             // and its length; 0: no run
  uint8_t  code;          // stage 1: 0, 1 a cap, 2 a refused input
  uint8_t  state;         // FLIST_ALIVE and the bits below
  uint16_t n_merged, total_edit;      // of gaps
};
static_assert(sizeof(FlistSlot) == 16, "one slot is 16 bytes");
constexpr uint32_t FLIST_NO_RECORD = 0xffffffffu;
constexpr uint8_t FLIST_ALIVE = 1, FLIST_HEAD = 2, FLIST_TAIL = 4, FLIST_BAD_GAPS = 8, FLIST_CAP_GAPS = 16, FLIST_UNORDERED = 32;

// The driver's device block for n ESTs, n_cands candidates and n_exons_total candidate exons.  Every exon array has
// n_exons_total + n_cands entries: the placeholder of candidate c is entry n_exons_total + c.  Offsets are multiples of
// 256; `total` bytes in all.
struct FlistLayout {
  size_t ex_in, ex_clean, ex_gaps, ex_kept, ex_refined;      // exon arrays: the candidates, then what each stage wrote
  size_t marks, gsteps, rsteps;                              // one byte per exon
  size_t cq, cr, gq, gr, rq, rr, slot;                       // per candidate: the three queries and results, the slot
  size_t res, need;                                          // per EST: the outcome; 3 words
  size_t cnt_f, cnt_e, first_f, first_e, scan_tmp;           // per EST (n + 1): the gather's two scans
  size_t facts, out_exons, out_steps;                        // the compact answer: at most n_cands facts, n_exons_total exons
  size_t total;
};
inline FlistLayout flist_layout(size_t n, size_t n_cands, size_t n_exons_total, size_t scan_tmp_bytes) {
  const size_t ne = n_exons_total + n_cands, exb = ne * sizeof(pgpu_factor);
  FlistLayout L;
  BlockCarver c;
  L.ex_in = c.take(exb); L.ex_clean = c.take(exb); L.ex_gaps = c.take(exb); L.ex_kept = c.take(exb); L.ex_refined = c.take(exb);
  L.marks = c.take(ne); L.gsteps = c.take(ne); L.rsteps = c.take(ne);
  L.cq = c.take(n_cands * sizeof(pgpu_clean_query)); L.cr = c.take(n_cands * sizeof(pgpu_clean_result));
  L.gq = c.take(n_cands * sizeof(pgpu_gaps_query)); L.gr = c.take(n_cands * sizeof(pgpu_gaps_result));
  L.rq = c.take(n_cands * sizeof(pgpu_chain_query)); L.rr = c.take(n_cands * sizeof(pgpu_chain_result));
  L.slot = c.take(n_cands * sizeof(FlistSlot));
  L.res = c.take(n * sizeof(pgpu_flist_result)); L.need = c.take(16);
  L.cnt_f = c.take((n + 1) * sizeof(uint32_t)); L.cnt_e = c.take((n + 1) * sizeof(uint32_t));
  L.first_f = c.take((n + 1) * sizeof(uint64_t)); L.first_e = c.take((n + 1) * sizeof(uint64_t)); L.scan_tmp = c.take(scan_tmp_bytes);
  L.facts = c.take(n_cands * sizeof(pgpu_flist_fact));
  L.out_exons = c.take(n_exons_total * sizeof(pgpu_factor)); L.out_steps = c.take(n_exons_total);
  L.total = c.at;
  return L;
}
