// The host side of the final stage that makes no HIP call, on the host alone (pintron_amd/csrc/pgpu_final.h): the validator
// of pgpu_index_final_factorizations, the validator of pgpu_pairing_plan_create_with_originals, and the layout of the final
// driver's device block.  Built with -fsanitize=address,undefined and run by tests/test_final_cpu.py; prints "ok" or the
// line that failed.
#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pintron_amd/csrc/pgpu_final.h"
#include "../../pintron_amd/csrc/pgpu_unit.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// One call: `q` over n_exons exons, ESTs of ests_len bytes.  The queries, the factorization queries and the table of named
// exons are heap blocks of exactly as many entries as there are, so that a read or a write past them is AddressSanitizer's
// to report.
static bool accepted(const std::vector<pgpu_final_query>& q, size_t n_exons, size_t ests_len = 100, std::vector<pgpu_fact_query>* fq_out = nullptr) {
  pgpu_final_query* const queries = (pgpu_final_query*)malloc(q.size() ? q.size() * sizeof(pgpu_final_query) : 1);
  for (size_t k = 0; k < q.size(); ++k) queries[k] = q[k];
  pgpu_fact_query* const fq = (pgpu_fact_query*)malloc(q.size() ? q.size() * sizeof(pgpu_fact_query) : 1);
  uint8_t* const named = (uint8_t*)calloc(n_exons ? n_exons : 1, 1);
  const bool ok = final_queries_ok(queries, q.size(), ests_len, n_exons, named, fq);
  if (fq_out) fq_out->assign(fq, fq + q.size());
  free(named); free(fq); free(queries);
  return ok;
}

static pgpu_final_query query(uint64_t est_off, uint32_t est_len, uint32_t first, uint32_t n, uint64_t orig_off) {
  pgpu_final_query x = {};
  x.est_off = est_off; x.est_len = est_len; x.first_exon = first; x.n_exons = n; x.orig_off = orig_off;
  return x;
}

// the originals of a plan, in heap blocks of exactly their sizes; the bytes themselves are never read
static const char* originals(const std::vector<uint64_t>& pat_off, const std::vector<uint32_t>& pat, const std::vector<uint64_t>& first,
                             bool bytes = true, bool lists = true) {
  uint64_t* const po = (uint64_t*)malloc(pat_off.size() * sizeof(uint64_t));
  memcpy(po, pat_off.data(), pat_off.size() * sizeof(uint64_t));
  uint32_t* const op = (uint32_t*)malloc(pat.size() ? pat.size() * sizeof(uint32_t) : 1);
  if (!pat.empty()) memcpy(op, pat.data(), pat.size() * sizeof(uint32_t));
  uint64_t* const of = (uint64_t*)malloc(first.size() ? first.size() * sizeof(uint64_t) : 1);
  if (!first.empty()) memcpy(of, first.data(), first.size() * sizeof(uint64_t));
  const char* const why = originals_wrong(po, pat_off.size() - 1, lists ? op : nullptr, lists ? of : nullptr, bytes ? "x" : nullptr, pat.size());
  free(of); free(op); free(po);
  return why;
}

int main() {
  static_assert(sizeof(pgpu_final_query) == 32 && sizeof(pgpu_final_result) == 32, "ABI layout");
  static_assert(offsetof(pgpu_final_result, outcome) == 0 && offsetof(pgpu_final_result, stage) == 1 && offsetof(pgpu_final_result, detail) == 2 &&
                offsetof(pgpu_final_result, first_exon) == 4 && offsetof(pgpu_final_result, n_exons) == 8 &&
                offsetof(pgpu_final_result, n_merged) == 10 && offsetof(pgpu_final_result, total_edit) == 12 &&
                offsetof(pgpu_final_result, tail_added) == 16 && offsetof(pgpu_final_result, polyA) == 20 &&
                offsetof(pgpu_final_result, polyadenil) == 21 && offsetof(pgpu_final_result, recovered) == 22 &&
                offsetof(pgpu_final_result, refused) == 23 && offsetof(pgpu_final_result, n_removed) == 24 &&
                offsetof(pgpu_final_result, n_added) == 26 && offsetof(pgpu_final_result, n_cleaned) == 28 &&
                offsetof(pgpu_final_result, prefix_added) == 30 && offsetof(pgpu_final_result, reserved) == 31, "result");
  // ---- the queries of the index form: three over five exons, the middle one without a candidate
  const std::vector<pgpu_final_query> three = { query(0, 50, 0, 3, 50), query(10, 20, 0xFFFFFFFFu, 0, 10), query(50, 50, 3, 2, 50) };
  {
    std::vector<pgpu_fact_query> fq;
    EXPECT(accepted(three, 5, 100, &fq));
    for (size_t k = 0; k < three.size(); ++k)
      EXPECT(fq[k].est_off == three[k].est_off && fq[k].est_len == three[k].est_len && fq[k].first_exon == three[k].first_exon &&
             fq[k].n_exons == three[k].n_exons && fq[k].reserved == 0);
  }
  EXPECT(accepted({}, 0, 0));
  { auto q = three; q[2].n_exons = 3; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[2].first_exon = 5; q[2].n_exons = 1; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[2].first_exon = 0xFFFFFFFFu; q[2].n_exons = 1; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[2].first_exon = 2; EXPECT(!accepted(q, 5)); }                               // exon 2 twice
  { auto q = three; q[2].est_off = 51; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[0].est_len = 101; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[1].est_len = 0; EXPECT(!accepted(q, 5)); }                                  // an empty EST, candidate or not
  { auto q = three; q[1].reserved = 1; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[1].est_off = ~(uint64_t)0; EXPECT(!accepted(q, 5)); }
  // the original sequence inside the buffer, with or without a candidate
  { auto q = three; q[0].orig_off = 50; EXPECT(accepted(q, 5)); }
  { auto q = three; q[0].orig_off = 51; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[1].orig_off = 80; EXPECT(accepted(q, 5)); }
  { auto q = three; q[1].orig_off = 81; EXPECT(!accepted(q, 5)); }
  { auto q = three; q[2].orig_off = ~(uint64_t)0; EXPECT(!accepted(q, 5)); }                      // no wrap of orig_off + est_len
  { auto q = three; q[2].orig_off = 100; EXPECT(!accepted(q, 5)); }
  // ---- the originals of a plan of four patterns of 10, 0, 7 and 5 bytes
  const std::vector<uint64_t> po = { 0, 10, 10, 17, 22 };
  EXPECT(originals(po, {}, {}) == nullptr);
  EXPECT(originals(po, {}, {}, false, false) == nullptr);                                         // n_orig == 0: nothing is looked at
  EXPECT(originals(po, { 0, 2, 3 }, { 4, 14, 21, 26 }) == nullptr);
  EXPECT(originals(po, { 1 }, { 0, 0 }, false) == nullptr);                                       // an empty original of an empty pattern: no byte
  EXPECT(originals(po, { 3 }, { 0, 5 }) == nullptr);
  EXPECT(originals(po, { 4 }, { 0, 5 }) != nullptr);                                              // an index >= n_pat
  EXPECT(originals(po, { 0xFFFFFFFFu }, { 0, 5 }) != nullptr);
  EXPECT(originals(po, { 2, 0 }, { 0, 7, 17 }) != nullptr);                                       // not ascending
  EXPECT(originals(po, { 2, 2 }, { 0, 7, 14 }) != nullptr);                                       // not strictly
  EXPECT(originals(po, { 0 }, { 0, 9 }) != nullptr);                                              // a length that differs
  EXPECT(originals(po, { 0 }, { 0, 11 }) != nullptr);
  EXPECT(originals(po, { 0, 2 }, { 0, 10, 3 }) != nullptr);                                       // offsets that go back
  EXPECT(originals(po, { 0 }, { 0, 10 }, false) != nullptr);                                      // null pointers with n_orig > 0
  EXPECT(originals(po, { 0 }, { 0, 10 }, true, false) != nullptr);
  // ---- the driver's device block: every part at a multiple of 256, no two parts overlap, the sizes as documented
  for (size_t n : { 1, 8, 9, 255, 256, 257 }) for (size_t e : { 0, 1, 16, 17, 1000 }) for (size_t scan : { 0, 1, 4096 }) {
    const FinalLayout L = final_layout(n, e, scan);
    const size_t ne = n + e;
    const size_t at[] = { L.ex_tin, L.ex_tout, L.ex_sin, L.ex_sout, L.tsteps, L.ssteps, L.tq, L.tr, L.sq, L.sr, L.res, L.counts, L.first,
                          L.scan_tmp, L.out_exons, L.out_steps, L.total };
    const size_t len[] = { ne * 16, ne * 16, ne * 16, 2 * ne * 16, ne, 2 * ne, n * 32, n * 16, n * 32, n * 24, n * 32, (n + 1) * 4, (n + 1) * 8,
                           scan, 2 * e * 16, 2 * e };
    EXPECT(at[0] == 0);
    for (int k = 0; k < 16; ++k) EXPECT(at[k] % 256 == 0 && at[k] + len[k] <= at[k + 1]);
    // the placeholder of the last EST and its list in small's output lie inside their arrays
    EXPECT((e + n - 1 + 1) * 16 <= L.ex_tout - L.ex_tin && (2 * (e + n - 1) + 2) * 16 <= L.tsteps - L.ex_sout);
  }
  // ---- the block carver (pgpu_layout.h) under the three stage layouts: no offset and no total moves.  Per row: n,
  // n_exons_total (for unit_layout: n_done_exons), then the 22 offsets of fact_layout, the 17 of final_layout and the 7 of
  // unit_layout in the order of their structs, at scan_tmp_bytes = 24; the literals were printed by the layouts as they
  // stood before the carver.
  {
    static const struct { size_t n, e, at[46]; } rows[] = {
    { 0, 0, { 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 4352, 4608, 4864, 5120, 5376, 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 0, 256, 512, 768, 1024, 1280, 1536 } },
    { 0, 1, { 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 4352, 4608, 4864, 5120, 5376, 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 0, 256, 512, 768, 1024, 1280, 1536 } },
    { 0, 300, { 0, 4864, 9728, 14592, 19456, 24320, 24832, 25344, 25856, 26112, 26368, 26624, 26880, 27136, 27392, 27648, 27904, 28160, 28416, 28672, 33536, 34048, 0, 4864, 9728, 14592, 24320, 24832, 25600, 25856, 26112, 26368, 26624, 26880, 27136, 27392, 27648, 37376, 38144, 0, 256, 512, 768, 1024, 1280, 6144 } },
    { 1, 0, { 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 4352, 4608, 4864, 5120, 5376, 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 0, 256, 512, 768, 1024, 1280, 1536 } },
    { 1, 1, { 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 4352, 4608, 4864, 5120, 5376, 0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 0, 256, 512, 768, 1024, 1280, 1536 } },
    { 1, 300, { 0, 4864, 9728, 14592, 19456, 24320, 24832, 25344, 25856, 26112, 26368, 26624, 26880, 27136, 27392, 27648, 27904, 28160, 28416, 28672, 33536, 34048, 0, 4864, 9728, 14592, 24320, 24832, 25600, 25856, 26112, 26368, 26624, 26880, 27136, 27392, 27648, 37376, 38144, 0, 256, 512, 768, 1024, 1280, 6144 } },
    { 255, 0, { 0, 4096, 8192, 12288, 16384, 20480, 20736, 20992, 21248, 29440, 33536, 39680, 43776, 54016, 58112, 62208, 62464, 63488, 65536, 65792, 66048, 66304, 0, 4096, 8192, 12288, 20480, 20736, 21248, 29440, 33536, 41728, 47872, 56064, 57088, 59136, 59392, 59648, 59904, 0, 4096, 10240, 11264, 13312, 13568, 16640 } },
    { 255, 1, { 0, 4096, 8192, 12288, 16384, 20480, 20736, 20992, 21248, 29440, 33536, 39680, 43776, 54016, 58112, 62208, 62464, 63488, 65536, 65792, 66048, 66304, 0, 4096, 8192, 12288, 20480, 20736, 21248, 29440, 33536, 41728, 47872, 56064, 57088, 59136, 59392, 59648, 59904, 0, 4096, 10240, 11264, 13312, 13568, 16896 } },
    { 255, 300, { 0, 8960, 17920, 26880, 35840, 44800, 45568, 46336, 47104, 55296, 59392, 65536, 69632, 79872, 83968, 88064, 88320, 89344, 91392, 91648, 96512, 97024, 0, 8960, 17920, 26880, 44800, 45568, 46848, 55040, 59136, 67328, 73472, 81664, 82688, 84736, 84992, 94720, 95488, 0, 4096, 10240, 11264, 13312, 13568, 21504 } },
    { 256, 0, { 0, 4096, 8192, 12288, 16384, 20480, 20736, 20992, 21248, 29440, 33536, 39680, 43776, 54016, 58112, 62208, 62464, 63744, 66048, 66304, 66560, 66816, 0, 4096, 8192, 12288, 20480, 20736, 21248, 29440, 33536, 41728, 47872, 56064, 57344, 59648, 59904, 60160, 60416, 0, 4096, 10240, 11520, 13824, 14080, 17152 } },
    { 256, 1, { 0, 4352, 8704, 13056, 17408, 21760, 22272, 22784, 23296, 31488, 35584, 41728, 45824, 56064, 60160, 64256, 64512, 65792, 68096, 68352, 68608, 68864, 0, 4352, 8704, 13056, 21504, 22016, 22784, 30976, 35072, 43264, 49408, 57600, 58880, 61184, 61440, 61696, 61952, 0, 4096, 10240, 11520, 13824, 14080, 17408 } },
    { 256, 300, { 0, 8960, 17920, 26880, 35840, 44800, 45568, 46336, 47104, 55296, 59392, 65536, 69632, 79872, 83968, 88064, 88320, 89600, 91904, 92160, 97024, 97536, 0, 8960, 17920, 26880, 44800, 45568, 46848, 55040, 59136, 67328, 73472, 81664, 82944, 85248, 85504, 95232, 96000, 0, 4096, 10240, 11520, 13824, 14080, 22016 } },
    { 257, 0, { 0, 4352, 8704, 13056, 17408, 21760, 22272, 22784, 23296, 31744, 36096, 42496, 46848, 57344, 61696, 66048, 66304, 67584, 69888, 70144, 70400, 70656, 0, 4352, 8704, 13056, 21504, 22016, 22784, 31232, 35584, 44032, 50432, 58880, 60160, 62464, 62720, 62976, 63232, 0, 4352, 10752, 12032, 14336, 14592, 17920 } },
    { 257, 1, { 0, 4352, 8704, 13056, 17408, 21760, 22272, 22784, 23296, 31744, 36096, 42496, 46848, 57344, 61696, 66048, 66304, 67584, 69888, 70144, 70400, 70656, 0, 4352, 8704, 13056, 21504, 22016, 22784, 31232, 35584, 44032, 50432, 58880, 60160, 62464, 62720, 62976, 63232, 0, 4352, 10752, 12032, 14336, 14592, 17920 } },
    { 257, 300, { 0, 8960, 17920, 26880, 35840, 44800, 45568, 46336, 47104, 55552, 59904, 66304, 70656, 81152, 85504, 89856, 90112, 91392, 93696, 93952, 98816, 99328, 0, 8960, 17920, 26880, 44800, 45568, 46848, 55296, 59648, 68096, 74496, 82944, 84224, 86528, 86784, 96512, 97280, 0, 4352, 10752, 12032, 14336, 14592, 22528 } },
    };
    EXPECT(sizeof rows / sizeof rows[0] == 15);
    for (const auto& r : rows) {
      const FactLayout A = fact_layout(r.n, r.e, 24);
      const FinalLayout B = final_layout(r.n, r.e, 24);
      const UnitLayout C = unit_layout(r.n, r.e, 24);
      const size_t got[46] = { A.ex_in, A.ex_clean, A.ex_gaps, A.ex_kept, A.ex_refined, A.marks, A.gsteps, A.rsteps, A.cq, A.cr, A.gq,
                               A.gr, A.rq, A.rr, A.res, A.need, A.counts, A.first, A.scan_tmp, A.out_exons, A.out_steps, A.total,
                               B.ex_tin, B.ex_tout, B.ex_sin, B.ex_sout, B.tsteps, B.ssteps, B.tq, B.tr, B.sq, B.sr, B.res, B.counts,
                               B.first, B.scan_tmp, B.out_exons, B.out_steps, B.total,
                               C.q, C.out, C.counts, C.first, C.scan_tmp, C.blob, C.total };
      for (int k = 0; k < 46; ++k) EXPECT(got[k] == r.at[k]);
    }
    BlockCarver c;
    EXPECT(c.take(0) == 0 && c.take(1) == 256 && c.take(256) == 512 && c.take(257) == 768 && c.at == 1280);
  }
  if (!failures) printf("ok\n");
  return failures != 0;
}
