// The parts of pintron_amd/csrc/pgpu_query_call.h that make no HIP call, on the host alone: the rounding of the
// device offsets, the return code of a HIP error, the range checks refine_introns and refine_chains share, and of the
// path the two chained entries share the validator (on both query structs) and the layout of the device block.
// Built with -fsanitize=address,undefined and run by tests/test_query_call_host.py; prints "ok" or the line that failed.
#include <limits.h>
#include <stdio.h>

#include "../../pintron_amd/csrc/pgpu_query_call.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// ---- the chained path.  One call: two queries over five exons, two ESTs of 50 bytes in a buffer of 100, a sequence of
// 1000 bytes.  `change` makes it the case under test; the exons and the table of named exons are heap blocks of exactly
// n_exons_total entries, so that a read or a write past them is AddressSanitizer's to report.
struct Sizes { size_t ests_len = 100, n_exons_total = 5, n = 2, glen = 1000; };

template <class Query, class Change, class Own>
static bool accepted(Change change, Own own) {
  const pgpu_factor five[5] = { { 0, 9, 100, 109 }, { 20, 29, 200, 209 }, { 40, 49, 300, 309 }, { 0, 9, 400, 409 }, { 20, 29, 500, 509 } };
  Query q[2] = {};
  q[0].est_len = 50; q[0].n_exons = 3;
  q[1].est_off = 50; q[1].est_len = 50; q[1].first_exon = 3; q[1].n_exons = 2;
  pgpu_factor ex[5];
  for (int k = 0; k < 5; ++k) ex[k] = five[k];
  Sizes c;
  change(c, q, ex);
  pgpu_factor* const exons = (pgpu_factor*)malloc(c.n_exons_total ? c.n_exons_total * sizeof(pgpu_factor) : 1);
  for (size_t k = 0; k < c.n_exons_total && k < 5; ++k) exons[k] = ex[k];
  uint8_t* const named = (uint8_t*)calloc(c.n_exons_total ? c.n_exons_total : 1, c.n_exons_total ? 1 : 0);
  const bool ok = chained_queries_ok(q, c.n, c.ests_len, exons, c.n_exons_total, c.glen, named, own);
  free(named);
  free(exons);
  return ok;
}

template <class Query>
static void check_chained_validator() {
  typedef Query* Q;
  typedef pgpu_factor* E;
  int calls = 0;
  const auto yes = [&](const Query&, const pgpu_factor*) { ++calls; return true; };
  EXPECT(accepted<Query>([](Sizes&, Q, E) {}, yes) && calls == 2);
  // refused, each for one reason alone; the entry's own rules are asked of no query whose common fields are bad
#define REFUSED(asked, ...) do { calls = 0; EXPECT(!accepted<Query>([](Sizes& c, Q q, E ex) { (void)c; (void)q; (void)ex; __VA_ARGS__; }, yes) && calls == asked); } while (0)
  REFUSED(1, q[1].n_exons = 0);
  REFUSED(1, q[1].first_exon = 5; q[1].n_exons = 1);                            // first_exon == n_exons_total
  REFUSED(1, q[1].first_exon = 0xFFFFFFFFu; q[1].n_exons = 1);                  // + n_exons wraps to 0 in 32 bits
  REFUSED(1, q[1].n_exons = 3);                                                 // one past the end
  REFUSED(0, c.n_exons_total = 3; c.n = 1; q[0].first_exon = 2; q[0].n_exons = 0xFFFFFFFFu);      // the sum wraps to 1
  REFUSED(1, q[1].est_off = 101);
  REFUSED(1, q[1].est_off = (uint64_t)1 << 40);
  REFUSED(1, c.ests_len = (size_t)1 << 32; q[1].est_len = 0x80000000u);         // inside its buffer, and too long
  REFUSED(1, q[1].est_len = 51);                                                // one more than what is left behind est_off
  REFUSED(0, q[0].est_len = 101);
  REFUSED(1, q[1].reserved = 1);
  REFUSED(0, q[0].reserved = 1);
  REFUSED(1, q[1].first_exon = 2);                                              // exon 2 is the first query's as well
  REFUSED(0, ex[1].GEN_end = 1001);                                             // a good range, its second exon past the sequence
  REFUSED(0, ex[1].EST_start = 51);
  REFUSED(0, c.n_exons_total = 0);
#undef REFUSED
  // a `false` from the entry's own rules refuses the call, at the query that gave it
  calls = 0;
  EXPECT(!accepted<Query>([](Sizes&, Q, E) {}, [&](const Query& x, const pgpu_factor*) { ++calls; return x.first_exon != 3; }) && calls == 2);
  calls = 0;
  EXPECT(!accepted<Query>([](Sizes&, Q, E) {}, [&](const Query&, const pgpu_factor*) { ++calls; return false; }) && calls == 1);
  // they see the query and its own first exon
  EXPECT(accepted<Query>([](Sizes&, Q, E) {}, [](const Query& x, const pgpu_factor* ex) { return ex[0].GEN_start == (x.first_exon ? 400 : 100); }));
}

static void check_chained_layout() {
  for (size_t ests_len : { 0, 1, 192, 193 }) for (size_t n_exons : { 0, 1, 16, 17 }) for (size_t n : { 1, 8, 9 })
    for (size_t extra : { 0, 256 }) for (size_t qsize : { sizeof(pgpu_chain_query), sizeof(pgpu_clean_query) }) {
      const size_t ws = 3 * 512;
      const ChainedLayout L = chained_layout(ests_len, n_exons, n, qsize, 16, extra, ws);
      // the parts in their order: where each begins and how many bytes it holds
      const size_t at[] = { 0, L.exons, L.queries, L.out_exons, L.out_bytes, L.results, L.extra, L.ws, L.total };
      const size_t len[] = { ests_len + 64, n_exons * 16, n * qsize, n_exons * 16, n_exons, n * 16, extra, ws };
      for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
      EXPECT(L.total == L.ws + ws && L.ws == L.extra + extra);
      EXPECT(L.ests_len == ests_len && L.ex_bytes == n_exons * 16 && L.q_bytes == n * qsize && L.n_exons == n_exons && L.r_bytes == n * 16);
    }
}

int main() {
  EXPECT(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
  EXPECT(up256(0 + 64) == 256 && up256(192 + 64) == 256 && up256(193 + 64) == 512);      // the slack behind a string buffer
  EXPECT(up256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);

  EXPECT(pgpu_code_of(hipErrorOutOfMemory) == PGPU_ENOMEM);
  EXPECT(pgpu_code_of(hipErrorInvalidValue) == PGPU_EDEVICE && pgpu_code_of(hipErrorIllegalAddress) == PGPU_EDEVICE &&
         pgpu_code_of(hipErrorLaunchFailure) == PGPU_EDEVICE && pgpu_code_of(hipErrorNoDevice) == PGPU_EDEVICE);

  EXPECT(coordinate_ok(-1, 0) && coordinate_ok(0, 0) && !coordinate_ok(1, 0) && !coordinate_ok(-2, 0));
  EXPECT(coordinate_ok(100, 100) && !coordinate_ok(101, 100) && !coordinate_ok(INT_MIN, 100));
  EXPECT(coordinate_ok(INT_MAX, (size_t)INT_MAX) && !coordinate_ok(INT_MAX, (size_t)INT_MAX - 1) && coordinate_ok(INT_MAX, (size_t)1 << 40));

  pgpu_factor f = { 0, 9, 100, 109 };
  EXPECT(factor_ok(f, 10, 110) && factor_ok(f, 9, 109) && !factor_ok(f, 8, 110) && !factor_ok(f, 10, 108));
  f.EST_start = -1; EXPECT(factor_ok(f, 10, 110));
  f.EST_start = -2; EXPECT(!factor_ok(f, 10, 110));
  f.EST_start = 11; EXPECT(!factor_ok(f, 10, 110));
  f.EST_start = 0; f.GEN_start = 111; EXPECT(!factor_ok(f, 10, 110));

  EXPECT(suffpref_ok(0, 0, 0) && suffpref_ok(30, 70, 30) && suffpref_ok(1 << 24, 1 << 24, 1 << 24));
  EXPECT(!suffpref_ok(-1, 70, 30) && !suffpref_ok(30, -1, 30) && !suffpref_ok(30, 70, -7));
  EXPECT(!suffpref_ok((1 << 24) + 1, 70, 30) && !suffpref_ok(30, (1 << 24) + 1, 30) && !suffpref_ok(30, 70, INT_MAX));

  check_chained_validator<pgpu_chain_query>();
  check_chained_validator<pgpu_clean_query>();
  const auto empty_est = [](Sizes& c, auto* q, pgpu_factor* ex) {               // no EST bytes at all, one query of two exons
    c.ests_len = 0; c.n = 1; c.n_exons_total = 2;
    q[0].est_len = 0; q[0].n_exons = 2;
    ex[0].EST_start = ex[0].EST_end = -1; ex[1].EST_start = ex[1].EST_end = 0;
  };
  EXPECT(accepted<pgpu_chain_query>(empty_est, [](const pgpu_chain_query&, const pgpu_factor*) { return true; }));
  EXPECT(!accepted<pgpu_clean_query>(empty_est, [](const pgpu_clean_query& x, const pgpu_factor*) { return x.est_len != 0; }));
  check_chained_layout();

  if (!failures) printf("ok\n");
  return failures != 0;
}
