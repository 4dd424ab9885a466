// The rules of pgpu_unit_records and of pgpu_pairing_plan_run_units on what a caller hands in (include/pintron_gpu.h), and
// the layout of the unit stage's device block: plain host code without a HIP call, in a header so that
// tests/hostcheck/unit_call_check.cpp runs the very code of the entries under the sanitizers.  Only structure is refused
// here: what the results and the exons say is judged per unit on the device (pgpu_unit.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_layout.h"

constexpr uint32_t UNIT_MAX_EXONS = 128;      // n_exons of a DONE pgpu_final_result
constexpr size_t UNIT_MAX_COUNT = 0x7fffffffull;
constexpr char UNIT_TOO_MANY[] = "more than 2^31 - 1 units or patterns in one call";

// The parameters: null when they are good, else what is wrong with them.
inline const char* unit_params_wrong(const pgpu_unit_params& p) {
  if (p.retain_externals > 1) return "bad unit parameters (retain_externals above 1)";
  if (p.reserved[0] || p.reserved[1] || p.reserved[2]) return "bad unit parameters (reserved != 0)";
  if (p.pref_N_length < 0 || p.pref_N_length > (1 << 30)) return "bad unit parameters (pref_N_length outside [0, 2^30])";
  return nullptr;
}

// The units over n_pat patterns: null when they are good.  `named`: n_pat bytes, all 0 on entry; a pattern a unit names is
// marked there.  No result is read.
inline const char* unit_queries_wrong(const pgpu_unit_query* q, size_t n, size_t n_pat, uint8_t* named) {
  if (n > UNIT_MAX_COUNT || n_pat > UNIT_MAX_COUNT) return UNIT_TOO_MANY;
  for (size_t i = 0; i < n; ++i) {
    const pgpu_unit_query& x = q[i];
    if (x.fwd >= n_pat) return "bad unit (fwd is no pattern)";
    if (x.rev != PGPU_UNIT_NO_SIBLING && x.rev >= n_pat) return "bad unit (rev is neither a pattern nor PGPU_UNIT_NO_SIBLING)";
    if (x.fwd == x.rev) return "bad unit (fwd == rev)";
    if (x.flags & ~(PGPU_UNIT_FWD_SUFF_POLYA | PGPU_UNIT_REV_SUFF_POLYA)) return "bad unit (flag bits beyond 0-1)";
    if (named[x.fwd] || (x.rev != PGPU_UNIT_NO_SIBLING && named[x.rev])) return "bad unit (a pattern named by two units)";
    named[x.fwd] = 1;
    if (x.rev != PGPU_UNIT_NO_SIBLING) named[x.rev] = 1;
  }
  return nullptr;
}

// The finals a caller of the form without a plan hands in: null when they are good.  No exon is read.
inline const char* unit_finals_wrong(const pgpu_final_result* res, size_t n_pat, size_t n_exons_total) {
  for (size_t i = 0; i < n_pat; ++i) {
    const pgpu_final_result& r = res[i];
    if (r.outcome > PGPU_FACT_DONE) return "bad final result (an outcome above 2)";
    if (r.outcome != PGPU_FACT_DONE) continue;
    if (r.n_exons == 0 || r.n_exons > UNIT_MAX_EXONS) return "bad final result (DONE with n_exons == 0 or above 128)";
    if (r.first_exon > n_exons_total || r.n_exons > n_exons_total - r.first_exon)
      return "bad final result (DONE with first_exon + n_exons beyond the exons)";
  }
  return nullptr;
}

// The exons of the DONE results (results that have passed unit_finals_wrong): two results may name the same exons, so
// this is not the size of the exon array.
inline size_t unit_finals_exons(const pgpu_final_result* res, size_t n_pat) {
  size_t sum = 0;
  for (size_t i = 0; i < n_pat; ++i) if (res[i].outcome == PGPU_FACT_DONE) sum += res[i].n_exons;
  return sum;
}

// The most bytes the groups of n units can take over finals whose DONE results have n_done_exons exons in all: a pattern is
// named by one unit at most, so every exon of a result is written once at most, behind 12 bytes of headers per unit.
inline size_t unit_blob_bound(size_t n, size_t n_done_exons) { return 12 * n + 16 * n_done_exons; }

// The stage's device block for n units.  Offsets are multiples of 256.
struct UnitLayout {
  size_t q, out;                      // per unit: the query, the result
  size_t counts, first, scan_tmp;     // per unit: the bytes of its group; the scan
  size_t blob;                        // the groups, compact, in unit order: unit_blob_bound bytes
  size_t total;
};
inline UnitLayout unit_layout(size_t n, size_t n_done_exons, size_t scan_tmp_bytes) {
  UnitLayout L;
  BlockCarver c;
  L.q = c.take(n * sizeof(pgpu_unit_query)); L.out = c.take(n * sizeof(pgpu_unit_result));
  L.counts = c.take((n + 1) * sizeof(uint32_t)); L.first = c.take((n + 1) * sizeof(uint64_t)); L.scan_tmp = c.take(scan_tmp_bytes);
  L.blob = c.take(unit_blob_bound(n, n_done_exons));
  L.total = c.at;
  return L;
}
