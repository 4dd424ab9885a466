// The host side of pgpu_index_small_chains that makes no HIP call, on the host alone: the validator the chained entries
// share (pintron_amd/csrc/pgpu_query_call.h) on pgpu_small_query with the entry's own rules (pintron_amd/csrc/pgpu_small.h)
// as its callable, the rule on the parameters, and the layout of the device block with two output slots per exon.  What
// tests/hostcheck/tail_call_check.cpp does for pgpu_tail_query.  Built with -fsanitize=address,undefined and run by
// tests/test_small_cpu.py; prints "ok" or the line that failed.
#include <limits.h>
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_query_call.h"
#include "../../pintron_amd/csrc/pgpu_small.h"

// chained_begin reports through the context; here there is none, and the code is what the check looks at
int pgpu_ctx_fail(pgpu_ctx*, int code, const char*) { return code; }

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// One call: `q` over `ex`, ESTs of ests_len bytes, a sequence of glen bytes.  The exons, the queries and the table of named
// exons are heap blocks of exactly as many entries as there are, so that a read or a write past them is AddressSanitizer's
// to report.
static bool accepted(const std::vector<pgpu_small_query>& q, const std::vector<pgpu_factor>& ex, size_t ests_len = 100, size_t glen = 1000) {
  const size_t n_exons = ex.size();
  pgpu_factor* const exons = (pgpu_factor*)malloc(n_exons ? n_exons * sizeof(pgpu_factor) : 1);
  for (size_t k = 0; k < n_exons; ++k) exons[k] = ex[k];
  pgpu_small_query* const queries = (pgpu_small_query*)malloc(q.size() ? q.size() * sizeof(pgpu_small_query) : 1);
  for (size_t k = 0; k < q.size(); ++k) queries[k] = q[k];
  uint8_t* const named = (uint8_t*)calloc(n_exons ? n_exons : 1, 1);
  const auto own = [=](const pgpu_small_query& x, const pgpu_factor* e) { return small_query_ok(x, e, ests_len, glen); };
  const bool ok = chained_queries_ok(queries, q.size(), ests_len, exons, n_exons, glen, named, own);
  free(named); free(queries); free(exons);
  return ok;
}

static pgpu_small_query query(uint64_t est_off, uint32_t est_len, uint32_t first, uint32_t n, uint64_t orig_off) {
  pgpu_small_query x = {};
  x.est_off = est_off; x.est_len = est_len; x.first_exon = first; x.n_exons = n; x.orig_off = orig_off;
  return x;
}

int main() {
  static_assert(sizeof(pgpu_small_query) == 32 && sizeof(pgpu_small_result) == 24 && sizeof(pgpu_small_params) == 8, "ABI layout");
  static_assert(offsetof(pgpu_small_result, status) == 0 && offsetof(pgpu_small_result, refused) == 4 && offsetof(pgpu_small_result, verdict) == 5 &&
                offsetof(pgpu_small_result, prefix_added) == 6 && offsetof(pgpu_small_result, reserved) == 7 &&
                offsetof(pgpu_small_result, n_added) == 8 && offsetof(pgpu_small_result, n_list) == 12 &&
                offsetof(pgpu_small_result, first_kept) == 16 && offsetof(pgpu_small_result, n_kept) == 20, "result");
  static_assert(offsetof(pgpu_small_params, min_intron_length) == 0 && offsetof(pgpu_small_params, reserved) == 4, "params");
  // the parameters: any min_intron_length, reserved 0
  {
    pgpu_small_params p = { 60, 0 };
    EXPECT(small_params_ok(&p));
    p.min_intron_length = INT_MIN; EXPECT(small_params_ok(&p));
    p.min_intron_length = INT_MAX; EXPECT(small_params_ok(&p));
    p.min_intron_length = 0; EXPECT(small_params_ok(&p));
    p.reserved = 1; EXPECT(!small_params_ok(&p));
    EXPECT(!small_params_ok(nullptr));
  }
  // two queries over five exons; the first has its original sequence behind its working one, the second uses one for both
  const std::vector<pgpu_factor> five = { { 0, 9, 100, 109 }, { 20, 29, 200, 209 }, { 40, 49, 300, 309 }, { 0, 9, 400, 409 }, { 20, 29, 500, 509 } };
  const std::vector<pgpu_small_query> two = { query(0, 50, 0, 3, 50), query(50, 50, 3, 2, 50) };
  EXPECT(accepted(two, five));
  // the common rules, each for one reason alone
  { auto q = two; q[1].n_exons = 0; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].n_exons = 3; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 5; q[1].n_exons = 1; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 0xFFFFFFFFu; q[1].n_exons = 1; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].first_exon = 2; EXPECT(!accepted(q, five)); }                              // exon 2 twice
  { auto q = two; q[1].est_off = 51; EXPECT(!accepted(q, five)); }
  { auto q = two; q[0].est_len = 101; EXPECT(!accepted(q, five)); }
  { auto q = two; q[1].reserved = 1; EXPECT(!accepted(q, five)); }
  // the entry's own rules at their edges: the original sequence inside the buffer
  { auto q = two; q[0].orig_off = 51; EXPECT(!accepted(q, five)); }
  { auto q = two; q[0].orig_off = 50; EXPECT(accepted(q, five)); }
  { auto q = two; q[0].orig_off = ~(uint64_t)0; EXPECT(!accepted(q, five)); }                      // no wrap of orig_off + est_len
  { auto q = two; q[1].est_len = 0; q[1].n_exons = 1; EXPECT(!accepted(q, five)); }                // an empty EST
  // ... every coordinate a byte of its string: the last accepted and the first refused value of each
  for (int field = 0; field < 4; ++field) {
    const int last = field < 2 ? 49 : 999;
    for (int which : { 0, 2, 4 }) {
      auto e = five;
      int32_t* const v = field == 0 ? &e[which].EST_start : field == 1 ? &e[which].EST_end : field == 2 ? &e[which].GEN_start : &e[which].GEN_end;
      *v = last; EXPECT(accepted(two, e));
      *v = last + 1; EXPECT(!accepted(two, e));
      *v = 0; EXPECT(accepted(two, e));
      *v = -1; EXPECT(!accepted(two, e));                                                        // what factor_ok lets pass
      *v = INT_MIN; EXPECT(!accepted(two, e));
      *v = INT_MAX; EXPECT(!accepted(two, e));
    }
  }
  // order is no rule of the input: the kernel refuses such a query (refused = 5)
  { auto e = five; e[1].EST_start = 9; EXPECT(accepted(two, e)); }
  { auto e = five; e[0] = { 9, 0, 109, 100 }; EXPECT(accepted(two, e)); }
  // the caps are the device's: 65 exons are good input
  {
    std::vector<pgpu_factor> many;
    for (int k = 0; k < 65; ++k) many.push_back({ k, k, 10 * k, 10 * k });
    EXPECT(accepted({ query(0, 65, 0, 65, 0) }, many, 65));
    many[64].EST_end = 65;
    EXPECT(!accepted({ query(0, 65, 0, 65, 0) }, many, 65));
  }
  // the device block for this struct: two output slots per exon, no flag slot, no workspace
  for (size_t ests_len : { 0, 1, 192, 193 }) for (size_t n_exons : { 1, 8, 9, 16, 17 }) for (size_t n : { 1, 8, 9 }) {
    const ChainedLayout L = chained_layout(ests_len, n_exons, n, sizeof(pgpu_small_query), sizeof(pgpu_small_result), 0, 0, 2);
    const size_t at[] = { 0, L.exons, L.queries, L.out_exons, L.out_bytes, L.results, L.extra, L.ws, L.total };
    const size_t len[] = { ests_len + 64, n_exons * 16, n * 32, 2 * n_exons * 16, 2 * n_exons, n * 24, 0, 0 };
    for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
    EXPECT(L.total == L.ws && L.ws == L.extra && L.q_bytes == n * 32 && L.r_bytes == n * 24 && L.out_per_exon == 2);
    // ... and the other entries' block is what it was
    const ChainedLayout L1 = chained_layout(ests_len, n_exons, n, sizeof(pgpu_tail_query), sizeof(pgpu_tail_result), 0, 0);
    EXPECT(L1.out_per_exon == 1 && L1.out_bytes == L1.out_exons + up256(n_exons * 16) && L1.results == L1.out_bytes + up256(n_exons));
  }
  // the empty call: both outputs all 0, twice the input's length, and not a byte more
  {
    NamedExons named;
    pgpu_factor ex[3] = { { 1, 2, 3, 4 }, { 5, 6, 7, 8 }, { 9, 10, 11, 12 } };
    pgpu_factor* const oe = (pgpu_factor*)malloc(6 * sizeof(pgpu_factor));
    uint8_t* const ob = (uint8_t*)malloc(6);
    memset(oe, 0xAB, 6 * sizeof(pgpu_factor)); memset(ob, 0xAB, 6);
    int dummy = 0;
    EXPECT(chained_begin((pgpu_ctx*)&dummy, (const pgpu_index*)&dummy, nullptr, 0, ex, 3, nullptr, 0, oe, ob, nullptr, "queries", named, 2) == PGPU_OK);
    for (int k = 0; k < 6; ++k) EXPECT(oe[k].EST_start == 0 && oe[k].EST_end == 0 && oe[k].GEN_start == 0 && oe[k].GEN_end == 0 && ob[k] == 0);
    free(oe); free(ob);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
