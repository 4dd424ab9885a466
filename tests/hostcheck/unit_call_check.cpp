// The host side of the unit stage that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_unit.h): the three
// validators of pgpu_unit_records and pgpu_pairing_plan_run_units and the layout of the stage's device block.  Built with
// -fsanitize=address,undefined and run by tests/test_unit_cpu.py; prints "ok" or the line that failed.
// With a file name as its argument it walks that blob of packed records with the reader of include/pintron_records.h
// instead and prints every number it meets, one group per line ("-1" when the reader refuses the blob).
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pintron_records.h"
#include "../../pintron_amd/csrc/pgpu_unit.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// The units over n_pat patterns, in heap blocks of exactly their sizes, so that a read or a write past them is
// AddressSanitizer's to report.
static const char* units_wrong(const std::vector<pgpu_unit_query>& q, size_t n_pat) {
  pgpu_unit_query* const queries = (pgpu_unit_query*)malloc(q.size() ? q.size() * sizeof(pgpu_unit_query) : 1);
  for (size_t k = 0; k < q.size(); ++k) queries[k] = q[k];
  uint8_t* const named = (uint8_t*)calloc(n_pat ? n_pat : 1, 1);
  const char* const why = unit_queries_wrong(queries, q.size(), n_pat, named);
  free(named); free(queries);
  return why;
}
static const char* finals_wrong(const std::vector<pgpu_final_result>& r, size_t n_exons_total) {
  pgpu_final_result* const res = (pgpu_final_result*)malloc(r.size() ? r.size() * sizeof(pgpu_final_result) : 1);
  for (size_t k = 0; k < r.size(); ++k) res[k] = r[k];
  const char* const why = unit_finals_wrong(res, r.size(), n_exons_total);
  free(res);
  return why;
}

static pgpu_unit_query unit(uint32_t est_index, uint32_t fwd, uint32_t rev, uint32_t flags) {
  pgpu_unit_query x = { est_index, fwd, rev, flags };
  return x;
}
static pgpu_final_result result(unsigned outcome, uint32_t first, unsigned n) {
  pgpu_final_result r;
  memset(&r, 0, sizeof r);
  r.outcome = (uint8_t)outcome; r.first_exon = first; r.n_exons = (uint16_t)n;
  return r;
}
static pgpu_unit_params params(int32_t pref, unsigned retain) {
  pgpu_unit_params p;
  memset(&p, 0, sizeof p);
  p.pref_N_length = pref; p.retain_externals = (uint8_t)retain;
  return p;
}

static int walk(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  std::vector<unsigned char> data;
  unsigned char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  unsigned char* const blob = (unsigned char*)malloc(data.size() ? data.size() : 1);      // exactly its size
  if (!data.empty()) memcpy(blob, data.data(), data.size());
  pfr_reader r;
  pfr_open(&r, blob, data.size());
  pfr_est e;
  int rc;
  while ((rc = pfr_next_est(&r, &e)) == 1) {
    printf("%u %u", e.est_index, e.n_factorizations);
    pfr_factorization x;
    int rf;
    while ((rf = pfr_next_factorization(&r, &x)) == 1) {
      printf(" %u %u %u", x.polya, x.polyad, x.n_exons);
      for (uint16_t k = 0; k < x.n_exons; ++k) {
        const pfr_exon ex = pfr_exon_at(&x, k);
        printf(" %d %d %d %d", ex.est_start, ex.est_end, ex.gen_start, ex.gen_end);
      }
    }
    printf("\n");
    if (rf < 0) { rc = -1; break; }
  }
  if (rc < 0) printf("-1\n");
  free(blob);
  return rc < 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return walk(argv[1]);
  static_assert(sizeof(pgpu_unit_query) == 16 && sizeof(pgpu_unit_params) == 8 && sizeof(pgpu_unit_result) == 24, "ABI layout");
  static_assert(offsetof(pgpu_unit_query, est_index) == 0 && offsetof(pgpu_unit_query, fwd) == 4 && offsetof(pgpu_unit_query, rev) == 8 &&
                offsetof(pgpu_unit_query, flags) == 12, "query");
  static_assert(offsetof(pgpu_unit_params, pref_N_length) == 0 && offsetof(pgpu_unit_params, retain_externals) == 4 &&
                offsetof(pgpu_unit_params, reserved) == 5, "params");
  static_assert(offsetof(pgpu_unit_result, verdict) == 0 && offsetof(pgpu_unit_result, strand) == 1 && offsetof(pgpu_unit_result, reason) == 2 &&
                offsetof(pgpu_unit_result, n_factorizations) == 3 && offsetof(pgpu_unit_result, pattern) == 4 &&
                offsetof(pgpu_unit_result, first_byte) == 8 && offsetof(pgpu_unit_result, n_bytes) == 16 &&
                offsetof(pgpu_unit_result, reserved) == 20, "result");
  const uint32_t NO = PGPU_UNIT_NO_SIBLING;
  // ---- the units: three over five patterns, the middle one without a sibling, in another order than their patterns
  const std::vector<pgpu_unit_query> three = { unit(7, 3, 4, 3), unit(0xFFFFFFFFu, 2, NO, 1), unit(0, 1, 0, 0) };
  EXPECT(units_wrong(three, 5) == nullptr);
  EXPECT(units_wrong({}, 0) == nullptr);
  EXPECT(units_wrong({}, 5) == nullptr);
  EXPECT(units_wrong({ unit(0, 0, NO, 0) }, 1) == nullptr);
  EXPECT(units_wrong({ unit(0, 0, NO, 0) }, 0) != nullptr);                                       // no pattern at all
  { auto q = three; q[0].fwd = 5; EXPECT(units_wrong(q, 5) != nullptr); }
  { auto q = three; q[0].fwd = NO; EXPECT(units_wrong(q, 5) != nullptr); }                        // NO_SIBLING is no forward pattern
  { auto q = three; q[0].rev = 5; EXPECT(units_wrong(q, 5) != nullptr); }
  { auto q = three; q[0].rev = NO - 1; EXPECT(units_wrong(q, 5) != nullptr); }
  { auto q = three; q[0].rev = 3; EXPECT(units_wrong(q, 5) != nullptr); }                         // fwd == rev
  { auto q = three; q[1].fwd = 4; EXPECT(units_wrong(q, 5) != nullptr); }                         // pattern 4 twice: rev, then fwd
  { auto q = three; q[2].rev = 3; EXPECT(units_wrong(q, 5) != nullptr); }                         // pattern 3 twice: fwd, then rev
  { auto q = three; q[2].fwd = 2; EXPECT(units_wrong(q, 5) != nullptr); }                         // fwd, then fwd
  { auto q = three; q[2].rev = 4; EXPECT(units_wrong(q, 5) != nullptr); }                         // rev, then rev
  { auto q = three; q[1].flags = 4; EXPECT(units_wrong(q, 5) != nullptr); }
  { auto q = three; q[1].flags = 0x80000001u; EXPECT(units_wrong(q, 5) != nullptr); }
  { auto q = three; q[1].flags = 2; EXPECT(units_wrong(q, 5) == nullptr); }                       // the sibling's bit without a sibling: a value
  { auto q = three; q[1].est_index = 0; q[2].est_index = 0; EXPECT(units_wrong(q, 5) == nullptr); }   // est_index is copied, never compared
  // the counts are looked at before any unit is
  EXPECT(unit_queries_wrong(nullptr, (size_t)1 << 31, 5, nullptr) != nullptr);
  EXPECT(unit_queries_wrong(nullptr, 0, (size_t)1 << 31, nullptr) != nullptr);
  // ---- the parameters
  EXPECT(unit_params_wrong(params(0, 0)) == nullptr && unit_params_wrong(params(0, 1)) == nullptr);
  EXPECT(unit_params_wrong(params(1 << 30, 1)) == nullptr);
  EXPECT(unit_params_wrong(params((1 << 30) + 1, 1)) != nullptr);
  EXPECT(unit_params_wrong(params(-1, 1)) != nullptr);
  EXPECT(unit_params_wrong(params(0, 2)) != nullptr && unit_params_wrong(params(0, 255)) != nullptr);
  for (int k = 0; k < 3; ++k) { pgpu_unit_params p = params(5, 1); p.reserved[k] = 1; EXPECT(unit_params_wrong(p) != nullptr); }
  // ---- the finals: four results over ten exons
  const std::vector<pgpu_final_result> four = { result(PGPU_FACT_DONE, 0, 4), result(PGPU_FACT_HOST, 99, 0), result(PGPU_FACT_EMPTY, 0, 7),
                                                result(PGPU_FACT_DONE, 4, 6) };
  EXPECT(finals_wrong(four, 10) == nullptr);
  EXPECT(finals_wrong({}, 0) == nullptr);
  EXPECT(finals_wrong(four, 9) != nullptr);
  { auto r = four; r[1].outcome = 3; EXPECT(finals_wrong(r, 10) != nullptr); }
  { auto r = four; r[1].outcome = 255; EXPECT(finals_wrong(r, 10) != nullptr); }
  { auto r = four; r[0].n_exons = 0; EXPECT(finals_wrong(r, 10) != nullptr); }
  { auto r = four; r[3].first_exon = 5; EXPECT(finals_wrong(r, 10) != nullptr); }
  { auto r = four; r[3].first_exon = 0xFFFFFFFFu; r[3].n_exons = 1; EXPECT(finals_wrong(r, 10) != nullptr); }   // no wrap
  { auto r = four; r[3].first_exon = 10; r[3].n_exons = 1; EXPECT(finals_wrong(r, 10) != nullptr); }
  { auto r = four; r[0].n_exons = 128; EXPECT(finals_wrong(r, 200) == nullptr); }
  { auto r = four; r[0].n_exons = 129; EXPECT(finals_wrong(r, 200) != nullptr); }
  // two results over the same exons are values: the blob's bound counts the exons of the results, not of the array
  { auto r = four; r[0].first_exon = 4; EXPECT(finals_wrong(r, 10) == nullptr && unit_finals_exons(r.data(), r.size()) == 10); }
  { auto r = four; r[0].first_exon = 4; r[3].first_exon = 2; EXPECT(finals_wrong(r, 8) == nullptr && unit_finals_exons(r.data(), r.size()) == 10); }
  EXPECT(unit_finals_exons(four.data(), 0) == 0 && unit_finals_exons(four.data(), 3) == 4);       // EMPTY with n_exons 7: not counted
  // ---- the block: every part at a multiple of 256, no two parts overlap, the sizes as documented, the bound
  EXPECT(unit_blob_bound(0, 0) == 0 && unit_blob_bound(3, 0) == 36 && unit_blob_bound(1, 128) == 12 + 2048);
  for (size_t n : { 1, 2, 255, 256, 257, 2049 }) for (size_t e : { 0, 1, 128, 1000 }) for (size_t scan : { 0, 1, 4096 }) {
    const UnitLayout L = unit_layout(n, e, scan);
    const size_t at[] = { L.q, L.out, L.counts, L.first, L.scan_tmp, L.blob, L.total };
    const size_t len[] = { n * 16, n * 24, (n + 1) * 4, (n + 1) * 8, scan, 12 * n + 16 * e };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 6; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
