// The host side of pgpu_index_candidate_lists that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_enum.h, the
// very code of the entry): the order of its refusals, its use of pgpu_index_candidates' validator on heap blocks of exactly
// the sizes named, and the arithmetic of its two device blocks -- results, candidate table, exons.  Built with
// -fsanitize=address,undefined and run by tests/test_enum_cpu.py; prints "ok" or the line that failed.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_enum.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef std::vector<uint8_t> Bytes;
struct Vertex { int32_t p, t, l; };
static const Vertex SOURCE = { CAND_SOURCE_P, CAND_SOURCE_P, CAND_MARK_LEN }, SINK = { CAND_SINK_P, CAND_SINK_P, CAND_MARK_LEN };

static void put(Bytes& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

static Bytes record(const std::vector<Vertex>& v, const std::vector<uint16_t>& first, const Bytes& tgt, uint32_t flags = 0) {
  Bytes b;
  const uint32_t head[4] = { (uint32_t)v.size(), (uint32_t)tgt.size(), flags, 0 };
  put(b, head, 16);
  for (const Vertex& x : v) put(b, &x, 12);
  for (uint16_t f : first) put(b, &f, 2);
  put(b, tgt.data(), tgt.size());
  while (b.size() & 3) b.push_back(0);
  const uint32_t texts[2] = { 0, 0 };
  put(b, texts, 8);
  return b;
}

// One call's refusal over the records laid end to end, on heap blocks of exactly the sizes named (one byte off alignment)
static int refusal(const std::vector<Bytes>& recs, pgpu_cand_params prm = { 15, 40 }, size_t glen = 1000, size_t n_override = (size_t)-1) {
  Bytes all;
  std::vector<uint64_t> first = { 0 };
  for (const Bytes& r : recs) { put(all, r.data(), r.size()); first.push_back(all.size()); }
  uint8_t* const block = (uint8_t*)malloc(all.size() + 1);
  for (size_t k = 0; k < all.size(); ++k) block[1 + k] = all[k];
  uint64_t* const off = (uint64_t*)malloc(first.size() * sizeof(uint64_t));
  for (size_t k = 0; k < first.size(); ++k) off[k] = first[k];
  size_t nc = 0, ne = 0;
  int token = 0;
  pgpu_enum_result out[8];
  const size_t n = n_override == (size_t)-1 ? recs.size() : n_override;
  const int rc = enum_call_refusal(&token, &token, block + 1, all.size(), off, n, &prm, out, nullptr, 0, nullptr, 0, &nc, &ne, glen);
  free(off); free(block);
  return rc;
}

static bool aligned(size_t x) { return (x & 255) == 0; }

int main() {
  static_assert(sizeof(pgpu_enum_result) == 16 && sizeof(pgpu_enum_candidate) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  static_assert(PGPU_ENUM_MAX_LIST == 64 && PGPU_ENUM_MAX_EMBEDDINGS == 512, "the caps");
  const std::vector<Vertex> five = { SOURCE, { 100, 200, 40 }, { 140, 500, 40 }, { 140, 600, 40 }, SINK };
  const Bytes branch = record(five, { 0, 1, 3, 4, 5, 5 }, { 1, 2, 3, 4, 4 });
  const Bytes cyclic = record(five, { 0, 1, 3, 4, 5, 5 }, { 1, 2, 3, 1, 4 });
  const Bytes bare = record({}, { 0 }, {}, PGPU_MEG_UNAVAILABLE);
  const Bytes empty_graph = record({ SOURCE, SINK }, { 0, 0, 0 }, {});
  // what the entry accepts: a branch, a cycle (CYCLIC is an answer, not a refusal), a flagged record, the empty graph, nothing
  EXPECT(refusal({ branch }) == ENUM_OK);
  EXPECT(refusal({ branch, cyclic, bare, empty_graph, record({}, { 0 }, {}) }) == ENUM_OK);
  EXPECT(refusal({}) == ENUM_OK);
  // the order of the refusals: a null pointer, the count, the parameters, the records
  {
    int token = 0;
    size_t nc = 0, ne = 0;
    const uint64_t off[2] = { 0, 16 };
    pgpu_cand_params prm = { 15, 40 }, bad = { 0, 40 };
    pgpu_enum_result out[1];
    pgpu_enum_candidate cd[1];
    pgpu_factor ex[1];
    const void* t = &token;
    EXPECT(enum_call_refusal(nullptr, t, bare.data(), 16, off, 1, &prm, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, nullptr, bare.data(), 16, off, 1, &prm, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, nullptr, 16, off, 1, &prm, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, nullptr, 1, &prm, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, nullptr, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, nullptr, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, out, nullptr, 1, ex, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, out, cd, 1, nullptr, 1, &nc, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, out, cd, 1, ex, 1, nullptr, &ne, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, out, cd, 1, ex, 1, &nc, nullptr, 10) == ENUM_NULL);
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, 1, &prm, out, nullptr, 0, nullptr, 0, &nc, &ne, 10) == ENUM_OK);      // no room asked for: no buffer needed
    EXPECT(enum_call_refusal(t, t, nullptr, 0, nullptr, 0, &prm, nullptr, nullptr, 0, nullptr, 0, &nc, &ne, 10) == ENUM_OK);   // the empty call
    EXPECT(enum_call_refusal(t, t, bare.data(), 16, off, (size_t)1 << 31, &bad, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_TOO_MANY);
    EXPECT(enum_call_refusal(t, t, bare.data(), 15, off, 1, &bad, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_PARAMS);              // before the records
    EXPECT(enum_call_refusal(t, t, bare.data(), 15, off, 1, &prm, out, cd, 1, ex, 1, &nc, &ne, 10) == ENUM_RECORDS);
  }
  { pgpu_cand_params p = { (1u << 24) + 1, 0 }; EXPECT(refusal({ branch }, p) == ENUM_PARAMS); p.min_factor_len = 1u << 24; EXPECT(refusal({ branch }, p) == ENUM_OK); }
  // the validator is the candidate stage's: every truncation point of a record with a branch (16 + 60 + 12 + 5 = 93 bytes)
  for (size_t cut = 0; cut < branch.size(); ++cut)
    EXPECT((refusal({ Bytes(branch.begin(), branch.begin() + cut) }) == ENUM_OK) == (cut >= 93));
  { Bytes r = branch; r[16 + 60 + 12 + 1] = 5; EXPECT(refusal({ r }) == ENUM_RECORDS); }                // a target that is no vertex
  { auto v = five; v[2] = { 140, 961, 40 }; EXPECT(refusal({ record(v, { 0, 1, 3, 4, 5, 5 }, { 1, 2, 3, 4, 4 }) }) == ENUM_RECORDS); }
  EXPECT(refusal({ branch, bare, Bytes(branch.begin(), branch.begin() + 92) }) == ENUM_RECORDS);      // a bad record behind good ones
  // the first block: ascending parts at multiples of 256 that hold what they must, the records at 0
  const size_t ns[] = { 0, 1, 63, 64, 65, 1000, 20000 };
  for (size_t n : ns)
    for (size_t rec_bytes : { (size_t)0, (size_t)16, (size_t)255, (size_t)256, (size_t)1000003 })
      for (size_t tmp : { (size_t)0, (size_t)1, (size_t)4096 }) {
        const EnumLayout L = enum_layout(rec_bytes, n, tmp);
        EXPECT(L.first >= rec_bytes + 4 && aligned(L.first));
        EXPECT(L.res >= L.first + (n + 1) * 8 && aligned(L.res));
        EXPECT(L.cnt_c >= L.res + n * sizeof(pgpu_enum_result) && L.cnt_c > L.res && aligned(L.cnt_c));
        EXPECT(L.cnt_e >= L.cnt_c + (n + 1) * 4 && aligned(L.cnt_e));
        EXPECT(L.off_c >= L.cnt_e + (n + 1) * 4 && aligned(L.off_c));
        EXPECT(L.off_e >= L.off_c + (n + 1) * 8 && aligned(L.off_e));
        EXPECT(L.tmp >= L.off_e + (n + 1) * 8 && aligned(L.tmp));
        EXPECT(L.total >= L.tmp + tmp && L.total > L.tmp && aligned(L.total));
        EXPECT(L.total <= up256(rec_bytes + 4) + (48 * n + 32) + tmp + 7 * 256);                 // nothing but padding beside them
      }
  // the second one: the candidate table, then the exons; an empty part has an address of its own
  for (size_t nc : { (size_t)0, (size_t)1, (size_t)16, (size_t)17, (size_t)512, (size_t)100000 })
    for (size_t ne : { (size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)32768, (size_t)1000000 }) {
      const EnumOutLayout O = enum_out_layout(nc, ne);
      EXPECT(O.cands == 0);
      EXPECT(O.exons >= nc * sizeof(pgpu_enum_candidate) && O.exons > O.cands && aligned(O.exons));
      EXPECT(O.total >= O.exons + ne * sizeof(pgpu_factor) && O.total > O.exons && aligned(O.total));
      EXPECT(O.total <= (nc + ne) * 16 + 3 * 256);
    }
  // the indices are 32 bits wide
  EXPECT(enum_totals_fit(0, 0) && enum_totals_fit(0xffffffffull, 0xffffffffull));
  EXPECT(!enum_totals_fit(0x100000000ull, 0) && !enum_totals_fit(0, 0x100000000ull));
  if (!failures) printf("ok\n");
  return failures != 0;
}
