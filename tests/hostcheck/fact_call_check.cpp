// The host side of pgpu_index_factorizations that makes no HIP call, on the host alone: the validator of the queries and
// the parameters, and the size arithmetic of the driver's device block (pintron_amd/csrc/pgpu_fact.h), the very code of
// the entry.  Every malformed query the header lists.  Built with -fsanitize=address,undefined and run by
// tests/test_fact_cpu.py; prints "ok" or the line that failed.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_fact.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// One call on heap blocks of exactly the sizes named, so that a read past them is AddressSanitizer's to report
static bool accepted(const std::vector<pgpu_fact_query>& q, size_t ests_len, size_t n_exons_total) {
  pgpu_fact_query* const block = (pgpu_fact_query*)malloc(q.size() * sizeof(pgpu_fact_query) + 1);
  for (size_t k = 0; k < q.size(); ++k) block[k] = q[k];
  uint8_t* const named = (uint8_t*)calloc(n_exons_total ? n_exons_total : 1, 1);
  const bool ok = fact_queries_ok(block, q.size(), ests_len, n_exons_total, named);
  free(named); free(block);
  return ok;
}

static pgpu_fact_query query(uint64_t est_off, uint32_t est_len, uint32_t first, uint32_t n, uint32_t reserved = 0) {
  pgpu_fact_query x;
  x.est_off = est_off; x.est_len = est_len; x.first_exon = first; x.n_exons = n; x.reserved = reserved;
  return x;
}

int main() {
  static_assert(sizeof(pgpu_fact_query) == 24 && sizeof(pgpu_fact_params) == 24 && sizeof(pgpu_fact_result) == 16, "ABI layout");
  static_assert(offsetof(pgpu_fact_result, detail) == 2 && offsetof(pgpu_fact_result, first_exon) == 4 &&
                offsetof(pgpu_fact_result, n_exons) == 8 && offsetof(pgpu_fact_result, n_merged) == 10 &&
                offsetof(pgpu_fact_result, total_edit) == 12, "ABI layout");
  // the parameters: the three suffpref lengths in [0, 2^24]; the threshold and min_intron_length are anything
  {
    pgpu_fact_params p = { 20.0, 30, 70, 30, 40 };
    EXPECT(fact_params_ok(p));
    p.suffpref_length_on_est = 0; p.suffpref_length_for_intron = 1 << 24; p.min_intron_length = INT_MIN; EXPECT(fact_params_ok(p));
    p.suffpref_length_for_intron = (1 << 24) + 1; EXPECT(!fact_params_ok(p));
    p.suffpref_length_for_intron = 70; p.suffpref_length_on_est = -1; EXPECT(!fact_params_ok(p));
    p.suffpref_length_on_est = 30; p.suffpref_length_on_gen = INT_MAX; EXPECT(!fact_params_ok(p));
    p.suffpref_length_on_gen = INT_MIN; EXPECT(!fact_params_ok(p));
    p.suffpref_length_on_gen = 30; p.complexity_threshold = -1e300; EXPECT(fact_params_ok(p));
  }
  // good batches
  EXPECT(accepted({}, 0, 0));
  EXPECT(accepted({ query(0, 100, 0, 3), query(100, 50, 3, 2) }, 150, 5));
  EXPECT(accepted({ query(0, 100, 3, 2), query(0, 100, 0, 3) }, 100, 5));              // one EST, two candidates, any order
  EXPECT(accepted({ query(0, 150, 0, 5) }, 150, 5));                                    // the whole of both buffers
  // no candidate: first_exon is not looked at, the EST is
  EXPECT(accepted({ query(0, 100, 0xFFFFFFFFu, 0), query(0, 100, 0, 0) }, 100, 0));
  EXPECT(!accepted({ query(0, 101, 0, 0) }, 100, 0));
  EXPECT(!accepted({ query(0, 0, 0, 0) }, 100, 0));
  // the EST's range
  EXPECT(!accepted({ query(0, 0, 0, 1) }, 100, 5));                                     // empty
  EXPECT(!accepted({ query(101, 1, 0, 1) }, 100, 5));
  EXPECT(!accepted({ query(100, 1, 0, 1) }, 100, 5));
  EXPECT(accepted({ query(99, 1, 0, 1) }, 100, 5));
  EXPECT(!accepted({ query(50, 51, 0, 1) }, 100, 5));
  EXPECT(!accepted({ query(~(uint64_t)0, 2, 0, 1) }, 100, 5));                          // est_off + est_len does not wrap
  EXPECT(!accepted({ query(0, 0x80000000u, 0, 1) }, (size_t)1 << 32, 5));               // beyond 2^31 - 1
  EXPECT(accepted({ query(0, 0x7fffffffu, 0, 1) }, (size_t)1 << 32, 5));
  EXPECT(!accepted({ query(0, 100, 0, 1, 1) }, 100, 5));                                // reserved
  // the candidate's range
  EXPECT(!accepted({ query(0, 100, 5, 1) }, 100, 5));
  EXPECT(!accepted({ query(0, 100, 6, 1) }, 100, 5));
  EXPECT(!accepted({ query(0, 100, 3, 3) }, 100, 5));
  EXPECT(!accepted({ query(0, 100, 0xFFFFFFFFu, 2) }, 100, 5));                         // first_exon + n_exons does not wrap
  EXPECT(!accepted({ query(0, 100, 1, 0xFFFFFFFFu) }, 100, 5));
  EXPECT(!accepted({ query(0, 100, 0, 1) }, 100, 0));
  // two queries share an exon
  EXPECT(!accepted({ query(0, 100, 0, 3), query(0, 100, 2, 2) }, 100, 5));
  EXPECT(!accepted({ query(0, 100, 0, 3), query(0, 100, 0, 3) }, 100, 5));
  EXPECT(accepted({ query(0, 100, 0, 2), query(0, 100, 2, 3) }, 100, 5));
  // a bad query behind good ones refuses the call
  EXPECT(!accepted({ query(0, 100, 0, 2), query(0, 100, 0, 0), query(0, 100, 2, 4) }, 100, 5));
  // the block: every part at a multiple of 256, in order, none overlapping, at the call's limits without overflow
  for (size_t n : { (size_t)0, (size_t)1, (size_t)65, (size_t)20000, (size_t)0x7fffffff }) {
    for (size_t e : { (size_t)0, (size_t)1, (size_t)100000, (size_t)0x7fffffff }) {
      const FactLayout L = fact_layout(n, e, 4096);
      const size_t at[] = { L.ex_in, L.ex_clean, L.ex_gaps, L.ex_kept, L.ex_refined, L.marks, L.gsteps, L.rsteps, L.cq, L.cr, L.gq,
                            L.gr, L.rq, L.rr, L.res, L.need, L.counts, L.first, L.scan_tmp, L.out_exons, L.out_steps, L.total };
      const size_t need[] = { (n + e) * 16, (n + e) * 16, (n + e) * 16, (n + e) * 16, (n + e) * 16, n + e, n + e, n + e, n * 32,
                              n * 16, n * 24, n * 16, n * 40, n * 16, n * 16, 12, (n + 1) * 4, (n + 1) * 8, 4096, e * 16, e };
      EXPECT(at[0] == 0);
      for (size_t k = 0; k + 1 < sizeof at / sizeof at[0]; ++k) {
        EXPECT(at[k] % 256 == 0);
        EXPECT(at[k + 1] >= at[k] + need[k] && at[k + 1] > at[k]);
      }
    }
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
