// The host side of the text stage that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_text.h): the two
// validators of pgpu_unit_texts and pgpu_pairing_plan_run_texts and the layouts of the stage's device blocks.  Built with
// -fsanitize=address,undefined and run by tests/test_text_cpu.py; prints "ok" or the line that failed.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_text.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// Offsets, units and blob in heap blocks of exactly their sizes, at an odd address for the blob, so that a read past them
// or a misaligned word read is the sanitizers' to report.
static const char* offsets_wrong(const std::vector<uint64_t>& first, size_t len) {
  uint64_t* const f = (uint64_t*)malloc(first.size() * sizeof(uint64_t));
  for (size_t k = 0; k < first.size(); ++k) f[k] = first[k];
  const char* const why = text_offsets_wrong(f, first.size() - 1, len, TEXT_BAD_HDR);
  free(f);
  return why;
}
static const char* units_wrong(const std::vector<pgpu_unit_result>& u, size_t n_pat, const std::vector<uint8_t>& blob) {
  pgpu_unit_result* const units = (pgpu_unit_result*)malloc(u.size() ? u.size() * sizeof(pgpu_unit_result) : 1);
  for (size_t k = 0; k < u.size(); ++k) units[k] = u[k];
  uint8_t* const b = (uint8_t*)malloc(blob.size() + 1);
  if (!blob.empty()) memcpy(b + 1, blob.data(), blob.size());
  const char* const why = text_units_wrong(units, u.size(), n_pat, b + 1, blob.size());
  free(b); free(units);
  return why;
}
static pgpu_unit_result unit(unsigned verdict, uint32_t pattern, uint64_t first_byte, uint32_t n_bytes) {
  pgpu_unit_result r;
  memset(&r, 0, sizeof r);
  r.verdict = (uint8_t)verdict; r.pattern = pattern; r.first_byte = first_byte; r.n_bytes = n_bytes;
  return r;
}
static void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
// a group: est_index, n_factorizations, then per factorization the header word and its exons
static void group(std::vector<uint8_t>& b, const std::vector<unsigned>& exons_per_fact) {
  put32(b, 7); put32(b, (uint32_t)exons_per_fact.size());
  for (unsigned n : exons_per_fact) {
    put32(b, 1u | n << 16);
    for (unsigned k = 0; k < 4 * n; ++k) put32(b, k);
  }
}

int main() {
  static_assert(sizeof(pgpu_text_result) == 32 && offsetof(pgpu_text_result, raw_first) == 0 && offsetof(pgpu_text_result, pests_first) == 8 &&
                offsetof(pgpu_text_result, raw_bytes) == 16 && offsetof(pgpu_text_result, pests_bytes) == 20 &&
                offsetof(pgpu_text_result, verdict) == 24 && offsetof(pgpu_text_result, reserved) == 25, "result");
  static_assert(PGPU_TEXT_MAX_UNIT_BYTES == 16777216u && PGPU_TEXT_NONE == 0u && PGPU_TEXT_DONE == 1u && PGPU_TEXT_HOST == 2u, "values");
  // ---- offsets: n + 1 of them, ascending, none past the length
  EXPECT(offsets_wrong({ 0 }, 0) == nullptr);
  EXPECT(offsets_wrong({ 0, 0, 0 }, 0) == nullptr);
  EXPECT(offsets_wrong({ 0, 3, 3, 10 }, 10) == nullptr);
  EXPECT(offsets_wrong({ 2, 3, 9 }, 10) == nullptr);                                   // need not begin at 0 nor end at the length
  EXPECT(offsets_wrong({ 0, 3, 2, 10 }, 10) != nullptr);
  EXPECT(offsets_wrong({ 0, 3, 11 }, 10) != nullptr);
  EXPECT(offsets_wrong({ 1 }, 0) != nullptr);
  EXPECT(offsets_wrong({ 5, 4 }, 10) != nullptr);
  EXPECT(offsets_wrong({ 0, ~(uint64_t)0 }, 10) != nullptr);
  // ---- units over a blob of three groups: 8 bytes; one factorization of 2 exons; factorizations of 0, 1 and 3 exons
  std::vector<uint8_t> blob;
  group(blob, {});
  const uint32_t g1 = (uint32_t)blob.size();
  group(blob, { 2 });
  const uint32_t g2 = (uint32_t)blob.size();
  group(blob, { 0, 1, 3 });
  const uint32_t end = (uint32_t)blob.size();
  EXPECT(g1 == 8 && g2 == 8 + 44 && end == g2 + 8 + 4 + 20 + 52);
  const std::vector<pgpu_unit_result> three = { unit(2, 4, g2, end - g2), unit(1, 99, 3, 5), unit(2, 0, 0, 8), unit(0, 99, 1, 1), unit(2, 1, g1, g2 - g1) };
  EXPECT(units_wrong(three, 5, blob) == nullptr);                                      // what is not ALIGNED is not looked at
  EXPECT(units_wrong({}, 0, {}) == nullptr);
  EXPECT(units_wrong({ unit(1, 0, 0, 0) }, 0, {}) == nullptr);
  { auto u = three; u[1].verdict = 3; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[3].verdict = 255; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[0].pattern = 5; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[0].pattern = 0xffffffffu; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[2].first_byte = 2; EXPECT(units_wrong(u, 5, blob) != nullptr); }            // no multiple of 4
  { auto u = three; u[2].n_bytes = 10; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[0].n_bytes += 4; EXPECT(units_wrong(u, 5, blob) != nullptr); }              // beyond the blob
  { auto u = three; u[0].first_byte = end; u[0].n_bytes = 8; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[0].first_byte = ~(uint64_t)0 - 3; EXPECT(units_wrong(u, 5, blob) != nullptr); }   // no wrap
  { auto u = three; u[0].first_byte = (uint64_t)1 << 32; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[2].n_bytes = 4; EXPECT(units_wrong(u, 5, blob) != nullptr); }               // shorter than a group's header
  { auto u = three; u[2].n_bytes = 0; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[4].n_bytes -= 4; EXPECT(units_wrong(u, 5, blob) != nullptr); }              // the exons pass n_bytes
  { auto u = three; u[4].n_bytes -= 16; EXPECT(units_wrong(u, 5, blob) != nullptr); }
  { auto u = three; u[2].n_bytes = 12; EXPECT(units_wrong(u, 5, blob) != nullptr); }              // bytes behind the last factorization
  { auto u = three; u[0].n_bytes -= 52; EXPECT(units_wrong(u, 5, blob) != nullptr); }             // a factorization is missing
  { auto u = three; u[0].first_byte = g1; u[0].n_bytes = end - g1; EXPECT(units_wrong(u, 5, blob) != nullptr); }   // two groups as one
  { auto b = blob; b[g1 + 4] = 2; EXPECT(units_wrong(three, 5, b) != nullptr); }                  // n_factorizations says more
  { auto b = blob; b[g1 + 4] = 0; EXPECT(units_wrong(three, 5, b) != nullptr); }                  // ... or fewer
  { auto b = blob; b[g1 + 10] = 3; EXPECT(units_wrong(three, 5, b) != nullptr); }                 // n_exons says more
  { auto b = blob; b[g1 + 11] = 0xff; EXPECT(units_wrong(three, 5, b) != nullptr); }
  { auto b = blob; b[4] = 0xff; b[5] = 0xff; b[6] = 0xff; b[7] = 0xff; EXPECT(units_wrong(three, 5, b) != nullptr); }   // 2^32 - 1 factorizations in 8 bytes
  // two units over the same group are values
  { auto u = three; u[2] = u[4]; EXPECT(units_wrong(u, 5, blob) == nullptr); }
  // the counts are looked at before any unit is
  EXPECT(text_units_wrong(nullptr, (size_t)1 << 31, 5, nullptr, 0) != nullptr);
  EXPECT(text_units_wrong(nullptr, 0, (size_t)1 << 31, nullptr, 0) != nullptr);
  // ---- the blocks: every part at a multiple of 256, no two parts overlap, 16 bytes behind what the copy loop reads
  for (size_t n : { 1, 2, 255, 256, 257, 2049 }) for (size_t h : { 0, 1, 240, 241, 100000 }) for (size_t scan : { 0, 1, 4096 }) {
    const TextLayout L = text_layout(n, h, scan);
    const size_t at[] = { L.hdr, L.hdr_first, L.out, L.raw_counts, L.raw_first, L.pests_counts, L.pests_first, L.scan_tmp, L.total };
    const size_t len[] = { h + 16, (n + 1) * 8, n * 32, (n + 1) * 4, (n + 1) * 8, (n + 1) * 4, (n + 1) * 8, scan };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 8; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
  }
  for (size_t n : { 1, 300 }) for (size_t b : { 0, 8, 4096 }) for (size_t s : { 0, 1, 255, 256, 70000 }) for (size_t p : { 1, 77 }) for (size_t g : { 0, 1, 200000 }) {
    const TextCallLayout L = text_call_layout(n, b, s, p, g);
    const size_t at[] = { L.units, L.blob, L.seqs, L.seq_first, L.genomic, L.stage };
    const size_t len[] = { n * 24, b + 16, s + 16, (p + 1) * 8, g + 16 };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 5; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
