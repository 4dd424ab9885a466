// The host side of pgpu_index_factorization_lists that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_flists.h,
// the very code of the entry): the order of its refusals, its validator on heap blocks of exactly the sizes named, and the
// arithmetic of its device block.  Built with -fsanitize=address,undefined and run by tests/test_flists_cpu.py; prints "ok"
// or the line that failed.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_flists.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static pgpu_flist_params good_params() {
  pgpu_flist_params p;
  memset(&p, 0, sizeof p);
  p.complexity_threshold = 20.0; p.suffpref_length_on_est = 30; p.suffpref_length_for_intron = 70; p.suffpref_length_on_gen = 30;
  p.min_intron_length = 40; p.max_coverage_diff = 0.05; p.max_site_difference = 50; p.max_gaplength_diff = 20;
  return p;
}

// One call's refusal with the queries, the candidates and the two tables on heap blocks of exactly the sizes named
static int refusal(const std::vector<pgpu_flist_query>& q, const std::vector<pgpu_enum_candidate>& c, size_t n_exons, size_t ests_len,
                   pgpu_flist_params prm = good_params()) {
  pgpu_flist_query* qq = (pgpu_flist_query*)malloc(q.size() * sizeof(pgpu_flist_query) + 1);
  pgpu_enum_candidate* cc = (pgpu_enum_candidate*)malloc(c.size() * sizeof(pgpu_enum_candidate) + 1);
  if (!q.empty()) memcpy(qq, q.data(), q.size() * sizeof(pgpu_flist_query));
  if (!c.empty()) memcpy(cc, c.data(), c.size() * sizeof(pgpu_enum_candidate));
  uint8_t* cn = (uint8_t*)calloc(c.size() ? c.size() : 1, 1);
  uint8_t* en = (uint8_t*)calloc(n_exons ? n_exons : 1, 1);
  int token = 0;
  size_t nf = 0, ne = 0;
  const void* t = &token;
  const int rc = flist_call_refusal(t, t, ests_len ? t : nullptr, ests_len, c.empty() ? nullptr : cc, c.size(), n_exons ? t : nullptr, n_exons,
                                    q.empty() ? nullptr : qq, q.size(), &prm, q.empty() ? nullptr : t, nullptr, 0, nullptr, nullptr, 0, &nf,
                                    &ne, cn, en);
  free(en); free(cn); free(cc); free(qq);
  return rc;
}

static pgpu_flist_query query(uint64_t off, uint32_t len, uint32_t first, uint32_t n, uint32_t reserved = 0) {
  pgpu_flist_query q; q.est_off = off; q.est_len = len; q.first_candidate = first; q.n_candidates = n; q.reserved = reserved; return q;
}
static pgpu_enum_candidate cand(uint32_t first, uint16_t n, uint32_t reserved = 0) {
  pgpu_enum_candidate c; c.first_exon = first; c.n_exons = n; c.n_pairs = 7; c.root = 99; c.reserved = reserved; return c;
}
static bool aligned(size_t x) { return (x & 255) == 0; }

int main() {
  static_assert(sizeof(pgpu_flist_params) == 48 && sizeof(pgpu_flist_query) == 24 && sizeof(pgpu_flist_result) == 16 &&
                sizeof(pgpu_flist_fact) == 16 && sizeof(FlistSlot) == 16, "ABI layout");
  static_assert(PGPU_FLIST_MAX_CANDIDATES == 64, "the cap");
  const std::vector<pgpu_enum_candidate> three = { cand(0, 2), cand(2, 3), cand(5, 1) };
  // what the entry accepts
  EXPECT(refusal({ query(0, 100, 0, 2), query(100, 50, 2, 1) }, three, 6, 150) == FLIST_OK);
  EXPECT(refusal({ query(0, 100, 0, 0), query(0, 100, 3, 0) }, three, 6, 150) == FLIST_OK);        // no candidate; the same EST twice
  EXPECT(refusal({}, {}, 0, 0) == FLIST_OK);
  EXPECT(refusal({ query(0, 100, 1, 2) }, { cand(0, 0, 5), cand(0, 2), cand(2, 4) }, 6, 100) == FLIST_OK);   // an unnamed candidate is not looked at
  // the queries
  EXPECT(refusal({ query(0, 0, 0, 1) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(51, 100, 0, 1) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(151, 0, 0, 1) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0, 1, 1) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 2, 2) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 4, 0) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0xffffffffu, 2) }, three, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0, 2), query(0, 100, 1, 2) }, three, 6, 150) == FLIST_QUERIES);      // two queries share a candidate
  // the candidates
  EXPECT(refusal({ query(0, 100, 0, 3) }, { cand(0, 2), cand(2, 0), cand(5, 1) }, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0, 3) }, { cand(0, 2), cand(2, 3, 1), cand(5, 1) }, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0, 3) }, { cand(0, 2), cand(2, 3), cand(5, 2) }, 6, 150) == FLIST_QUERIES);
  EXPECT(refusal({ query(0, 100, 0, 3) }, { cand(0, 2), cand(1, 3), cand(5, 1) }, 6, 150) == FLIST_QUERIES);   // two candidates share an exon
  EXPECT(refusal({ query(0, 100, 0, 1) }, { cand(7, 1) }, 6, 150) == FLIST_QUERIES);
  // the parameters, in front of the queries
  {
    pgpu_flist_params p = good_params();
    p.max_coverage_diff = 1.0; EXPECT(refusal({ query(0, 0, 0, 1) }, three, 6, 150, p) == FLIST_QUERIES);
    p.max_coverage_diff = 1.0000001; EXPECT(refusal({ query(0, 0, 0, 1) }, three, 6, 150, p) == FLIST_PARAMS);
    p.max_coverage_diff = -1e-9; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p.max_coverage_diff = NAN; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.max_site_difference = -1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.max_site_difference = (1 << 24) + 1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.max_site_difference = 1 << 24; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_OK);
    p = good_params(); p.max_gaplength_diff = -2; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.max_gaplength_diff = -1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_OK);
    p = good_params(); p.max_number_of_factorizations = -1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.max_number_of_factorizations = (1 << 24) + 1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.suffpref_length_on_gen = -1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
    p = good_params(); p.reserved = 1; EXPECT(refusal({}, {}, 0, 0, p) == FLIST_PARAMS);
  }
  // the order: a null pointer, the counts, the parameters, the queries
  {
    int token = 0;
    const void* t = &token;
    size_t nf = 0, ne = 0;
    pgpu_flist_params p = good_params(), bad = good_params();
    bad.reserved = 1;
    pgpu_flist_query q1 = query(0, 0, 0, 1);
    pgpu_enum_candidate c1 = cand(0, 1);
    uint8_t cn[1] = { 0 }, en[1] = { 0 };
    EXPECT(flist_call_refusal(nullptr, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, nullptr, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, nullptr, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, nullptr, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, nullptr, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, nullptr, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, nullptr, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, nullptr, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, nullptr, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, nullptr, t, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, nullptr, 1, &nf, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, nullptr, &ne, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, nullptr, cn, en) == FLIST_NULL);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, (size_t)1 << 31, &bad, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_TOO_MANY);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, (size_t)1 << 31, t, 1, &q1, 1, &bad, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_TOO_MANY);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, (size_t)1 << 31, &q1, 1, &bad, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_TOO_MANY);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &bad, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_PARAMS);       // before the queries
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, t, 1, t, t, 1, &nf, &ne, cn, en) == FLIST_QUERIES);
    EXPECT(flist_call_refusal(t, t, t, 10, &c1, 1, t, 1, &q1, 1, &p, t, nullptr, 0, nullptr, nullptr, 0, &nf, &ne, cn, en) == FLIST_QUERIES);   // no room asked for: no buffer needed
  }
  // the block: ascending parts at multiples of 256 that hold what they must
  for (size_t n : { (size_t)0, (size_t)1, (size_t)64, (size_t)1000 })
    for (size_t nc : { (size_t)0, (size_t)1, (size_t)65, (size_t)20000 })
      for (size_t ne : { (size_t)0, (size_t)1, (size_t)17, (size_t)300000 })
        for (size_t tmp : { (size_t)0, (size_t)4096 }) {
          const FlistLayout L = flist_layout(n, nc, ne, tmp);
          const size_t exb = (ne + nc) * 16;
          const size_t parts[] = { L.ex_in, L.ex_clean, L.ex_gaps, L.ex_kept, L.ex_refined, L.marks, L.gsteps, L.rsteps, L.cq, L.cr, L.gq, L.gr,
                                   L.rq, L.rr, L.slot, L.res, L.need, L.cnt_f, L.cnt_e, L.first_f, L.first_e, L.scan_tmp, L.facts,
                                   L.out_exons, L.out_steps, L.total };
          const size_t sizes[] = { exb, exb, exb, exb, exb, ne + nc, ne + nc, ne + nc, nc * 32, nc * 16, nc * 24, nc * 16, nc * 40, nc * 16,
                                   nc * 16, n * 16, 16, (n + 1) * 4, (n + 1) * 4, (n + 1) * 8, (n + 1) * 8, tmp, nc * 16, ne * 16, ne };
          EXPECT(parts[0] == 0);
          size_t sum = 0;
          for (int k = 0; k < 25; ++k) {
            EXPECT(aligned(parts[k]) && parts[k + 1] >= parts[k] + sizes[k] && parts[k + 1] > parts[k]);
            sum += sizes[k];
          }
          EXPECT(aligned(L.total) && L.total <= sum + 25 * 256);                 // nothing but padding beside them
        }
  if (!failures) printf("ok\n");
  return failures != 0;
}
