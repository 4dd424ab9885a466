// The host side of pgpu_index_gap_chains that makes no HIP call, on the host alone: the validator the chained entries
// share (pintron_amd/csrc/pgpu_query_call.h) on pgpu_gaps_query with the entry's own rules (pintron_amd/csrc/pgpu_gaps.h)
// as its callable, and the layout of the device block for that struct.  What tests/hostcheck/query_call_check.cpp does
// for the two other chained structs.  Built with -fsanitize=address,undefined and run by tests/test_gaps_cpu.py; prints
// "ok" or the line that failed.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_query_call.h"
#include "../../pintron_amd/csrc/pgpu_gaps.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// One call: `q` over `ex`, ESTs of ests_len bytes, a sequence of glen bytes.  The exons and the table of named exons are
// heap blocks of exactly as many entries as there are exons, so that a read or a write past them is AddressSanitizer's
// to report.
static bool accepted(const std::vector<pgpu_gaps_query>& q, const std::vector<pgpu_factor>& ex, size_t ests_len = 100, size_t glen = 1000) {
  const size_t n_exons = ex.size();
  pgpu_factor* const exons = (pgpu_factor*)malloc(n_exons ? n_exons * sizeof(pgpu_factor) : 1);
  for (size_t k = 0; k < n_exons; ++k) exons[k] = ex[k];
  pgpu_gaps_query* const queries = (pgpu_gaps_query*)malloc(q.size() ? q.size() * sizeof(pgpu_gaps_query) : 1);
  for (size_t k = 0; k < q.size(); ++k) queries[k] = q[k];
  uint8_t* const named = (uint8_t*)calloc(n_exons ? n_exons : 1, 1);
  const bool ok = chained_queries_ok(queries, q.size(), ests_len, exons, n_exons, glen, named, gaps_query_ok);
  free(named); free(queries); free(exons);
  return ok;
}

static pgpu_gaps_query query(uint64_t est_off, uint32_t est_len, uint32_t first, uint32_t n) {
  pgpu_gaps_query x = {};
  x.est_off = est_off; x.est_len = est_len; x.first_exon = first; x.n_exons = n;
  return x;
}

int main() {
  static_assert(sizeof(pgpu_gaps_query) == 24 && sizeof(pgpu_gaps_result) == 16, "ABI layout");
  // two queries over five exons, two ESTs of 50 bytes; gaps of 10 EST bytes over 90 genomic ones
  const std::vector<pgpu_factor> five = { { 0, 9, 100, 109 }, { 20, 29, 200, 209 }, { 40, 49, 300, 309 }, { 0, 9, 400, 409 }, { 20, 29, 500, 509 } };
  const std::vector<pgpu_gaps_query> two = { query(0, 50, 0, 3), query(50, 50, 3, 2) };
  EXPECT(accepted(two, five));
  // the common rules, each for one reason alone
  { auto q = two; q[1].n_exons = 0; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].n_exons = 3; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 5; q[1].n_exons = 1; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 0xFFFFFFFFu; q[1].n_exons = 1; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 2; EXPECT(!accepted(q, five)); }                              // exon 2 twice
  { auto q = two; q[1].est_off = 51; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].est_off = (uint64_t)1 << 40; EXPECT(!accepted(q, five)); }
  { auto q = two; q[0].est_len = 101; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].reserved = 1; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].est_len = 0x80000000u; EXPECT(!accepted(q, five, (size_t)1 << 32)); }     // inside its buffer, and too long
  { auto q = two; q[1].est_len = 0x7fffffffu; EXPECT(accepted(q, five, (size_t)1 << 32)); }
  { auto e = five; e[1].GEN_end = 1001; EXPECT(!accepted(two, e)); }
  { auto e = five; e[1].EST_start = -2; EXPECT(!accepted(two, e)); }
  { auto e = five; e[4].EST_end = 51; EXPECT(!accepted(two, e)); }
  EXPECT(!accepted(two, {}));
  // the entry's own rules at their edges
  { auto q = two; q[1].est_len = 0; q[1].n_exons = 1; auto e = five; e[3] = { -1, -1, 400, 409 }; EXPECT(!accepted(q, e)); }      // an empty EST
  { auto e = five; e[1].EST_start = 10; EXPECT(accepted(two, e)); }                              // no EST gap
  { auto e = five; e[1].EST_start = 9; EXPECT(!accepted(two, e)); }                              // EST_end == the next EST_start
  { auto e = five; e[1].EST_start = 8; EXPECT(!accepted(two, e)); }
  { auto e = five; e[1].GEN_start = 110; EXPECT(!accepted(two, e)); }                            // ten EST bytes over no genomic gap
  { auto e = five; e[1].EST_start = 10; e[1].GEN_start = 110; EXPECT(accepted(two, e)); }        // no gap on either string
  { auto e = five; e[1].EST_start = 10; e[1].GEN_start = 109; EXPECT(!accepted(two, e)); }       // GEN_end == the next GEN_start
  { auto e = five; e[1].GEN_start = 120; EXPECT(accepted(two, e)); }                             // gapP == gapT == 10
  { auto e = five; e[1].GEN_start = 119; EXPECT(!accepted(two, e)); }                            // gapP == gapT + 1
  { auto e = five; e[4].GEN_start = 420; EXPECT(accepted(two, e)); }                             // ... in the last pair of the last query
  { auto e = five; e[4].GEN_start = 419; EXPECT(!accepted(two, e)); }
  { auto e = five; e[0] = { -1, -1, -1, -1 }; EXPECT(accepted(two, e)); }                        // an exon of unset ends in front: gaps of 20 over 200
  { auto e = five; e[2] = { 50, 50, 1000, 1000 }; EXPECT(accepted(two, e)); }                    // the last exon behind both strings
  // the coordinates at the ends of int32: the gap lengths do not wrap
  {
    const std::vector<pgpu_factor> wide = { { -1, -1, -1, -1 }, { INT_MAX, INT_MAX, INT_MAX, INT_MAX } };
    EXPECT(accepted({ query(0, 0x7fffffffu, 0, 2) }, wide, (size_t)INT_MAX, (size_t)INT_MAX));
    const std::vector<pgpu_factor> wide2 = { { -1, -1, -1, 0 }, { INT_MAX, INT_MAX, INT_MAX, INT_MAX } };
    EXPECT(!accepted({ query(0, 0x7fffffffu, 0, 2) }, wide2, (size_t)INT_MAX, (size_t)INT_MAX));
  }
  // the caps are the device's: 65 exons, or an EST gap of 65 bytes, are good input
  {
    std::vector<pgpu_factor> many;
    for (int k = 0; k < 65; ++k) many.push_back({ k, k, 10 * k, 10 * k });
    EXPECT(accepted({ query(0, 65, 0, 65) }, many, 65));
    many[64].EST_start = many[64].EST_end = 63;                                                  // the last pair out of order
    EXPECT(!accepted({ query(0, 65, 0, 65) }, many, 65));
    const std::vector<pgpu_factor> far = { { 0, 9, 100, 109 }, { 75, 80, 300, 309 } };
    EXPECT(accepted({ query(0, 100, 0, 2) }, far));
  }
  // the device block for this struct: no flag slot, no workspace
  for (size_t ests_len : { 0, 1, 192, 193 }) for (size_t n_exons : { 1, 16, 17 }) for (size_t n : { 1, 10, 11 }) {
    const ChainedLayout L = chained_layout(ests_len, n_exons, n, sizeof(pgpu_gaps_query), sizeof(pgpu_gaps_result), 0, 0);
    const size_t at[] = { 0, L.exons, L.queries, L.out_exons, L.out_bytes, L.results, L.extra, L.ws, L.total };
    const size_t len[] = { ests_len + 64, n_exons * 16, n * 24, n_exons * 16, n_exons, n * 16, 0, 0 };
    for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
    EXPECT(L.total == L.ws && L.ws == L.extra && L.q_bytes == n * 24 && L.r_bytes == n * 16);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
