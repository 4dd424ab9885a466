// The host side of the side stage that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_side.h): the validators
// of pgpu_unit_sides and the layouts of the stage's device blocks.  Built with -fsanitize=address,undefined and run by
// tests/test_side_cpu.py; prints "ok" or the line that failed.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_side.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
// a record of nv vertices and ne edges with texts of ml and xl bytes, padded to 4; `claim_*`: what its lengths say
static void record(std::vector<uint8_t>& b, uint32_t nv, uint32_t ne, uint32_t flags, uint32_t ml, uint32_t xl, uint32_t claim_ml,
                   uint32_t claim_xl) {
  put32(b, nv); put32(b, ne); put32(b, flags); put32(b, 0);
  for (uint32_t k = 0; k < 12 * nv + 2 * (nv + 1) + ne; ++k) b.push_back((uint8_t)k);
  while (b.size() & 3) b.push_back(0);
  put32(b, claim_ml); put32(b, claim_xl);
  for (uint32_t k = 0; k < ml + xl; ++k) b.push_back((uint8_t)('a' + k % 26));
  while (b.size() & 3) b.push_back(0);
}
static void bare(std::vector<uint8_t>& b, uint32_t flags) { put32(b, 0); put32(b, 0); put32(b, flags); put32(b, 0); }

struct Batch {
  std::vector<uint8_t> recs;
  std::vector<uint64_t> first;
  std::vector<pgpu_unit_query> q;
  std::vector<pgpu_unit_result> u;
};
// Offsets, units and records in heap blocks of exactly their sizes, the record blob at an odd address, so that a read past
// them or a misaligned word read is the sanitizers' to report.
static const char* wrong(const Batch& B) {
  const size_t n = B.q.size(), n_pat = B.first.size() - 1;
  pgpu_unit_query* const q = (pgpu_unit_query*)malloc(n ? n * sizeof *q : 1);
  pgpu_unit_result* const u = (pgpu_unit_result*)malloc(n ? n * sizeof *u : 1);
  for (size_t k = 0; k < n; ++k) { q[k] = B.q[k]; u[k] = B.u[k]; }
  uint64_t* const f = (uint64_t*)malloc(B.first.size() * sizeof *f);
  for (size_t k = 0; k < B.first.size(); ++k) f[k] = B.first[k];
  uint8_t* const r = (uint8_t*)malloc(B.recs.size() + 1);
  if (!B.recs.empty()) memcpy(r + 1, B.recs.data(), B.recs.size());
  const char* why = side_records_wrong(f, n_pat, B.recs.size());
  if (!why) why = side_units_wrong(q, u, n, r + 1, f, n_pat);
  free(r); free(f); free(u); free(q);
  return why;
}
static pgpu_unit_query query(uint32_t fwd, uint32_t rev) { pgpu_unit_query x; memset(&x, 0, sizeof x); x.fwd = fwd; x.rev = rev; return x; }
static pgpu_unit_result unit(unsigned verdict, unsigned strand, uint32_t pattern) {
  pgpu_unit_result r;
  memset(&r, 0, sizeof r);
  r.verdict = (uint8_t)verdict; r.strand = (uint8_t)strand; r.pattern = pattern;
  return r;
}

int main() {
  static_assert(sizeof(pgpu_side_result) == 40 && offsetof(pgpu_side_result, megs_first) == 0 && offsetof(pgpu_side_result, pmegs_first) == 8 &&
                offsetof(pgpu_side_result, edges_first) == 16 && offsetof(pgpu_side_result, megs_bytes) == 24 &&
                offsetof(pgpu_side_result, pmegs_bytes) == 28 && offsetof(pgpu_side_result, edges_bytes) == 32 &&
                offsetof(pgpu_side_result, verdict) == 36 && offsetof(pgpu_side_result, reserved) == 37, "result");
  static_assert(PGPU_SIDE_MAX_UNIT_BYTES == 16777216u && PGPU_SIDE_NONE == 0u && PGPU_SIDE_DONE == 1u && PGPU_SIDE_HOST == 2u, "values");
  const uint32_t NO = PGPU_UNIT_NO_SIBLING;
  // six patterns: 0 a graph with texts, 1 the empty graph, 2 unavailable, 3 too complex, 4 texts of 0 bytes, 5 the last one
  Batch good;
  const uint32_t shape[6][5] = { { 5, 4, 0, 61, 33 }, { 2, 0, 0, 70, 0 }, { 0, 0, PGPU_MEG_UNAVAILABLE, 0, 0 },
                                 { 3, 2, PGPU_MEG_TOO_COMPLEX, 40, 7 }, { 2, 1, 0, 0, 0 }, { 64, 200, 0, 1001, 999 } };
  for (const auto& s : shape) {
    good.first.push_back(good.recs.size());
    if (s[2] & PGPU_MEG_UNAVAILABLE) bare(good.recs, s[2]);
    else record(good.recs, s[0], s[1], s[2], s[3], s[4], s[3], s[4]);
  }
  good.first.push_back(good.recs.size());
  good.q = { query(0, 1), query(4, NO), query(2, 3), query(5, 0), query(1, 4), query(3, NO) };
  good.u = { unit(2, 1, 1), unit(1, 0, 4), unit(0, 1, 3), unit(2, 0, 5), unit(1, 1, 4), unit(0, 0, 3) };
  EXPECT(wrong(good) == nullptr);                                                      // a HOST unit may name flagged records
  { Batch b; b.first = { 0 }; EXPECT(wrong(b) == nullptr); }
  // ---- the record offsets
  { Batch b = good; b.first[2] += 2; EXPECT(wrong(b) != nullptr); }                    // no multiple of 4
  { Batch b = good; b.first[6] += 4; EXPECT(wrong(b) != nullptr); }                    // past recs_len
  { Batch b = good; b.first[3] = b.first[2] - 4; EXPECT(wrong(b) != nullptr); }        // do not ascend
  { Batch b = good; b.first[6] = ~(uint64_t)0 - 3; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.recs.pop_back(); EXPECT(wrong(b) != nullptr); }
  // ---- the units
  { Batch b = good; b.u[1].verdict = 3; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.u[5].verdict = 255; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.u[1].strand = 2; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.q[1].fwd = 6; b.u[1].pattern = 6; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.q[0].rev = 6; b.u[0].pattern = 6; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.q[3].rev = 0xfffffffeu; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.u[1].strand = 1; b.u[1].pattern = NO; EXPECT(wrong(b) != nullptr); }        // strand 1 without a sibling
  { Batch b = good; b.u[5].strand = 1; b.u[5].pattern = NO; EXPECT(wrong(b) != nullptr); }        // ... on a HOST unit too
  { Batch b = good; b.u[0].pattern = 0; EXPECT(wrong(b) != nullptr); }                            // the other strand's pattern
  { Batch b = good; b.u[3].pattern = 4; EXPECT(wrong(b) != nullptr); }
  { Batch b = good; b.u[2].pattern = 2; EXPECT(wrong(b) != nullptr); }                            // ... on a HOST unit too
  // ---- a settled unit over a flagged record
  { Batch b = good; b.u[2].verdict = 1; EXPECT(wrong(b) != nullptr); }                            // fwd unavailable
  { Batch b = good; b.u[5].verdict = 2; EXPECT(wrong(b) != nullptr); }                            // fwd too complex
  { Batch b = good; b.q[0] = query(0, 3); b.u[0].pattern = 3; EXPECT(wrong(b) != nullptr); }      // the sibling is flagged
  { Batch b = good; b.q[3] = query(5, 2); EXPECT(wrong(b) == nullptr); }                          // strand 0: the sibling is not read
  // ---- a settled unit over a record that does not add up
  for (int which = 0; which < 4; ++which) {
    Batch b;
    b.first = { 0 };
    if (which == 0) record(b.recs, 4, 3, 0, 10, 10, 10, 11 + 2);         // the texts pass the record's padding
    if (which == 1) record(b.recs, 4, 3, 0, 10, 10, 0xfffffff0u, 0x20u); // lengths whose sum wraps in 32 bits
    if (which == 2) { put32(b.recs, 4); put32(b.recs, 3); put32(b.recs, 0); put32(b.recs, 0); for (int k = 0; k < 60; ++k) b.recs.push_back(0); }   // no room for the lengths
    if (which == 3) { put32(b.recs, 0xffffffffu); put32(b.recs, 0xffffffffu); put32(b.recs, 0); put32(b.recs, 0); put32(b.recs, 0); put32(b.recs, 0); }
    b.first.push_back(b.recs.size());
    b.q = { query(0, NO) }; b.u = { unit(1, 0, 0) };
    EXPECT(wrong(b) != nullptr);
    b.u[0].verdict = 0;
    EXPECT(wrong(b) == nullptr);                                         // a HOST unit's records are not read
  }
  { Batch b; b.first = { 0, 12 }; b.recs.assign(12, 0); b.q = { query(0, NO) }; b.u = { unit(2, 0, 0) }; EXPECT(wrong(b) != nullptr); }   // shorter than a header
  { Batch b; b.first = { 0, 0 }; b.q = { query(0, NO) }; b.u = { unit(2, 0, 0) }; EXPECT(wrong(b) != nullptr); }                          // an empty record
  {                                                                      // texts that end exactly with the record: good
    Batch b;
    b.first = { 0 };
    record(b.recs, 3, 2, 0, 9, 7, 9, 7);
    b.first.push_back(b.recs.size());
    b.q = { query(0, NO) }; b.u = { unit(2, 0, 0) };
    EXPECT(wrong(b) == nullptr);
    Batch c = b;
    c.first[1] -= 4;                                                     // the next record begins inside this one's texts
    c.recs.resize(c.recs.size() - 4);
    EXPECT(wrong(c) != nullptr);
  }
  // the counts are looked at before any unit is
  EXPECT(side_units_wrong(nullptr, nullptr, (size_t)1 << 31, nullptr, nullptr, 5) != nullptr);
  EXPECT(side_units_wrong(nullptr, nullptr, 0, nullptr, nullptr, (size_t)1 << 31) != nullptr);
  // ---- the blocks: every part at a multiple of 256, no two parts overlap, 16 bytes behind what the copy loop reads
  for (size_t n : { 1, 2, 255, 256, 257, 2049 }) for (size_t scan : { 0, 1, 4096 }) {
    const SideLayout L = side_layout(n, scan);
    const size_t at[] = { L.out, L.counts[0], L.first[0], L.counts[1], L.first[1], L.counts[2], L.first[2], L.scan_tmp, L.total };
    const size_t len[] = { n * 40, (n + 1) * 4, (n + 1) * 8, (n + 1) * 4, (n + 1) * 8, (n + 1) * 4, (n + 1) * 8, scan };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
  }
  for (size_t n : { 1, 300 }) for (size_t r : { 0, 16, 4096 }) for (size_t p : { 1, 77 }) for (size_t h : { 0, 1, 255, 256 }) for (size_t s : { 0, 1, 70000 }) {
    const SideCallLayout L = side_call_layout(n, r, p, h, s);
    const size_t at[] = { L.q, L.units, L.recs, L.rec_first, L.hdr, L.hdr_first, L.seqs, L.seq_first, L.stage };
    const size_t len[] = { n * 16, n * 24, r + 16, (p + 1) * 8, h + 16, (n + 1) * 8, s + 16, (p + 1) * 8 };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
  }
  for (unsigned long long a : { 0ull, 1ull, 256ull, 16777216ull }) for (unsigned long long b : { 0ull, 255ull }) for (unsigned long long c : { 0ull, 257ull }) {
    const unsigned long long t[3] = { a, b, c };
    const SideBlobs S = side_blobs(t);
    EXPECT(S.at[0] == 0 && S.at[0] + a <= S.at[1] && S.at[1] + b <= S.at[2] && S.at[2] + c <= S.total);
    EXPECT(S.at[1] % 256 == 0 && S.at[2] % 256 == 0 && S.at[0] != S.at[1] && S.at[1] != S.at[2]);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
