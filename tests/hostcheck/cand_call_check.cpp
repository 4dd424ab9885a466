// The host side of pgpu_index_candidates that makes no HIP call, on the host alone: the validator of the records a caller
// hands in (pintron_amd/csrc/pgpu_cand.h), the very code of the entry.  Every malformed record the header lists, and every
// truncation point of a valid one.  Built with -fsanitize=address,undefined and run by tests/test_cand_cpu.py; prints "ok"
// or the line that failed.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_cand.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef std::vector<uint8_t> Bytes;
struct Vertex { int32_t p, t, l; };
static const Vertex SOURCE = { CAND_SOURCE_P, CAND_SOURCE_P, CAND_MARK_LEN }, SINK = { CAND_SINK_P, CAND_SINK_P, CAND_MARK_LEN };

static void put(Bytes& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

// a record: header, vertices, CSR offsets, targets, padding, two empty texts
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

// One call over the records laid end to end (or at the offsets given), on heap blocks of exactly the sizes named, so that a
// read past them is AddressSanitizer's to report.  The buffer is handed over one byte off alignment: only offsets count.
static bool accepted(const std::vector<Bytes>& recs, size_t glen = 1000, const std::vector<uint64_t>* offsets = nullptr,
                     size_t records_len = (size_t)-1) {
  Bytes all;
  std::vector<uint64_t> first = { 0 };
  for (const Bytes& r : recs) { put(all, r.data(), r.size()); first.push_back(all.size()); }
  if (offsets) first = *offsets;
  if (records_len == (size_t)-1) records_len = all.size();
  uint8_t* const block = (uint8_t*)malloc(all.size() + 1);
  for (size_t k = 0; k < all.size(); ++k) block[1 + k] = all[k];
  uint64_t* const off = (uint64_t*)malloc(first.size() * sizeof(uint64_t));
  for (size_t k = 0; k < first.size(); ++k) off[k] = first[k];
  const bool ok = cand_records_ok(block + 1, records_len, off, first.size() - 1, glen);
  free(off); free(block);
  return ok;
}

int main() {
  static_assert(sizeof(pgpu_cand_params) == 8 && sizeof(pgpu_cand_result) == 16, "ABI layout");
  const std::vector<Vertex> four = { SOURCE, { 100, 200, 40 }, { 140, 500, 40 }, SINK };
  const std::vector<uint16_t> csr = { 0, 1, 2, 3, 3 };
  const Bytes tgt = { 1, 2, 3 };
  const Bytes good = record(four, csr, tgt);
  const Bytes bare = record({}, { 0 }, {}, PGPU_MEG_UNAVAILABLE);
  EXPECT(accepted({ good }));
  EXPECT(accepted({ good, bare, good }));
  EXPECT(accepted({}));
  // the parameters
  { pgpu_cand_params p = { 15, 40 }; EXPECT(cand_params_ok(p)); p.min_factor_len = 0; EXPECT(!cand_params_ok(p));
    p.min_factor_len = 1u << 24; EXPECT(cand_params_ok(p)); p.min_factor_len = (1u << 24) + 1; EXPECT(!cand_params_ok(p));
    p.min_factor_len = 1; p.min_intron_length = INT_MIN; EXPECT(cand_params_ok(p)); }
  // every truncation point of a valid record: the graph part (16 + 48 + 10 + 3 = 77 bytes) is what the entry needs
  for (size_t cut = 0; cut < good.size(); ++cut) {
    const Bytes part(good.begin(), good.begin() + cut);
    EXPECT(accepted({ part }) == (cut >= 77));
  }
  // ... and of a flagged one, whose 16 bytes are all that is read
  for (size_t cut = 0; cut <= 16; ++cut) EXPECT(accepted({ Bytes(bare.begin(), bare.begin() + cut) }) == (cut == 16));
  { Bytes huge = bare; const uint32_t n = 0xFFFFFFFFu; memcpy(huge.data(), &n, 4); memcpy(huge.data() + 4, &n, 4); EXPECT(accepted({ huge })); }
  { Bytes both = bare; both[8] = 3; EXPECT(accepted({ both })); both[8] = PGPU_MEG_TOO_COMPLEX; EXPECT(accepted({ both })); }
  // the offsets
  { const std::vector<uint64_t> o = { 0, good.size(), good.size() - 4 }; EXPECT(!accepted({ good, good }, 1000, &o)); }              // not ascending
  { const std::vector<uint64_t> o = { 0, good.size() + 4 }; EXPECT(!accepted({ good }, 1000, &o)); }                                // beyond records_len
  { const std::vector<uint64_t> o = { 0, good.size() }; EXPECT(!accepted({ good }, 1000, &o, good.size() - 1)); }
  { const std::vector<uint64_t> o = { (uint64_t)1 << 40, ((uint64_t)1 << 40) + 16 }; EXPECT(!accepted({ good }, 1000, &o)); }
  { const std::vector<uint64_t> o = { ~(uint64_t)0 - 3, 16 }; EXPECT(!accepted({ good }, 1000, &o)); }
  for (uint64_t shift = 1; shift < 4; ++shift) {                                                                                    // not at a multiple of 4
    Bytes lead(shift, 0);
    const std::vector<uint64_t> o = { shift, shift + good.size() };
    EXPECT(!accepted({ lead, good }, 1000, &o));
  }
  { Bytes lead(4, 0); const std::vector<uint64_t> o = { 4, 4 + good.size() }; EXPECT(accepted({ lead, good }, 1000, &o)); }
  { const std::vector<uint64_t> o = { 0, 0 }; EXPECT(!accepted({ good }, 1000, &o)); }                                              // an empty record
  // the counts
  {
    std::vector<Vertex> many = { SOURCE };
    for (int k = 0; k < 62; ++k) many.push_back({ 10 * k, 10 * k, 10 });
    many.push_back(SINK);
    std::vector<uint16_t> f; Bytes t;
    for (int k = 0; k < 64; ++k) { f.push_back((uint16_t)k); if (k < 63) t.push_back((uint8_t)(k + 1)); }
    f.push_back(63);
    EXPECT(accepted({ record(many, f, t) }));
    many.insert(many.begin() + 1, Vertex{ 0, 0, 0 });                                                   // 65 vertices
    f.push_back(63);
    EXPECT(!accepted({ record(many, f, t) }));
    Bytes flagged = record(many, f, t, PGPU_MEG_TOO_COMPLEX);                                    // ... under a flag nothing of it is read
    EXPECT(accepted({ flagged }));
  }
  { Bytes r = good; const uint32_t ne = 0xFFFFFFFFu; memcpy(r.data() + 4, &ne, 4); EXPECT(!accepted({ r })); }                      // n_edges beyond the record
  { Bytes r = good; const uint32_t ne = (uint32_t)good.size() - 74 + 1; memcpy(r.data() + 4, &ne, 4); EXPECT(!accepted({ r })); }
  { Bytes r = good; const uint32_t ne = 2; memcpy(r.data() + 4, &ne, 4); EXPECT(!accepted({ r })); }                                // the CSR goes beyond n_edges
  // the CSR offsets and the targets
  { auto f = csr; f[2] = 0; EXPECT(!accepted({ record(four, f, tgt) })); }                                                          // not ascending
  { auto f = csr; f[4] = 4; EXPECT(!accepted({ record(four, f, tgt) })); }
  { auto f = csr; f[0] = 1; EXPECT(accepted({ record(four, f, tgt) })); }                                                           // an edge nobody owns
  { auto f = csr; f[0] = 0xFFFF; EXPECT(!accepted({ record(four, f, tgt) })); }
  { auto t = tgt; t[1] = 4; EXPECT(!accepted({ record(four, csr, t) })); }
  { auto t = tgt; t[2] = 255; EXPECT(!accepted({ record(four, csr, t) })); }
  { auto t = tgt; t[0] = 0; EXPECT(accepted({ record(four, csr, t) })); }                                                           // a cycle is good input
  { auto f = csr; f = { 0, 3, 3, 3, 3 }; EXPECT(accepted({ record(four, f, tgt) })); }                                              // a branch too
  { EXPECT(accepted({ record({}, { 0 }, {}) })); EXPECT(accepted({ record({ SOURCE }, { 0, 0 }, {}) })); }                          // no path, and good input
  // the vertices
  const auto with = [&](size_t k, Vertex v) { auto x = four; x[k] = v; return record(x, csr, tgt); };
  EXPECT(accepted({ with(1, { 100, 960, 40 }) }));                                  // ends on the sequence's last byte
  EXPECT(!accepted({ with(1, { 100, 961, 40 }) }));
  EXPECT(accepted({ with(1, { 100, 1000, 0 }) }));
  EXPECT(!accepted({ with(1, { 100, 1001, 0 }) }));
  EXPECT(!accepted({ with(1, { 100, -1, 40 }) }));
  EXPECT(!accepted({ with(2, { 100, 200, -1 }) }));
  EXPECT(!accepted({ with(2, { -1, 200, 40 }) }));
  EXPECT(accepted({ with(2, { 0, 0, 0 }) }));
  EXPECT(!accepted({ with(2, { 100, INT_MAX, 1 }) }, (size_t)INT_MAX));             // t + l does not wrap
  EXPECT(accepted({ with(2, { 100, INT_MAX - 1, 1 }) }, (size_t)INT_MAX));
  EXPECT(accepted({ with(2, { (1 << 29) - 40, 200, 40 }) }));                      // p + l at its bound
  EXPECT(!accepted({ with(2, { (1 << 29) - 39, 200, 40 }) }));
  EXPECT(!accepted({ with(2, { INT_MAX, 200, 40 }) }));
  EXPECT(!accepted({ with(2, { 0, 0, INT_MAX }) }, (size_t)INT_MAX));
  EXPECT(accepted({ with(2, { 0, 0, 1 << 29 }) }, (size_t)INT_MAX));
  EXPECT(accepted({ with(1, SINK) })); EXPECT(accepted({ with(2, SOURCE) }));       // a second source or sink: no path, good input
  EXPECT(!accepted({ with(0, { CAND_SOURCE_P, 0, CAND_MARK_LEN }) }));
  EXPECT(!accepted({ with(0, { CAND_SOURCE_P, CAND_SOURCE_P, 199 }) }));
  EXPECT(!accepted({ with(3, { CAND_SINK_P, CAND_SINK_P, 201 }) }));
  EXPECT(!accepted({ with(3, { CAND_SINK_P, 5, CAND_MARK_LEN }) }));
  EXPECT(!accepted({ with(3, { CAND_SINK_P + 1, CAND_SINK_P, CAND_MARK_LEN }) }));  // not the sink's p: a pairing beyond its bounds
  // a bad record behind good ones refuses the call
  EXPECT(!accepted({ good, bare, with(1, { 100, 961, 40 }) }));
  if (!failures) printf("ok\n");
  return failures != 0;
}
