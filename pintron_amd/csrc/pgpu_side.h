// The rules of pgpu_unit_sides on what a caller hands in (include/pintron_gpu.h), and the layout of the side stage's device
// block: plain host code without a HIP call, in a header so that tests/hostcheck/side_call_check.cpp runs the very code of
// the entry under the sanitizers.  Only structure is refused here.  The plan form hands in what the device made and has no
// use for these checks: there the count pass (pgpu_side.hip) guards the same things and answers PGPU_SIDE_HOST.
// processed-megs-info.txt (per-EST microseconds) is not part of the stage.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_layout.h"
#include "pgpu_text.h"

constexpr char SIDE_BAD_REC[] = "bad record offsets (they do not ascend, pass recs_len, or are no multiple of 4)";
constexpr char SIDE_NO_SPACE[] = "side buffers too small";

// n_pat + 1 record offsets into recs_len bytes: null when they are good
inline const char* side_records_wrong(const uint64_t* rec_first, size_t n_pat, size_t recs_len) {
  if (text_offsets_wrong(rec_first, n_pat, recs_len, SIDE_BAD_REC)) return SIDE_BAD_REC;
  for (size_t i = 0; i <= n_pat; ++i)
    if (rec_first[i] & 3) return SIDE_BAD_REC;
  return nullptr;
}

// Record x (offsets that have passed side_records_wrong) as a settled unit needs it: null when it is not flagged and its
// graph part, its 8 bytes of lengths and its two texts end at or before rec_first[x + 1].  The blob is read with memcpy: a
// caller's buffer may lie anywhere.
inline const char* side_record_wrong(const void* recs, const uint64_t* rec_first, size_t x) {
  const uint8_t* const R = (const uint8_t*)recs + rec_first[x];
  const uint64_t len = rec_first[x + 1] - rec_first[x];
  if (len < 16) return "bad record (shorter than its 16 bytes of header)";
  uint32_t h[3];
  memcpy(h, R, 12);
  if (h[2] & (PGPU_MEG_TOO_COMPLEX | PGPU_MEG_UNAVAILABLE)) return "bad unit (a settled unit names a flagged record)";
  const uint64_t graph = (16 + 12 * (uint64_t)h[0] + 2 * ((uint64_t)h[0] + 1) + h[1] + 3) & ~(uint64_t)3;
  if (graph + 8 > len) return "bad record (its graph and text lengths pass the next record)";
  uint32_t t[2];
  memcpy(t, R + graph, 8);
  if ((uint64_t)t[0] + t[1] > len - graph - 8) return "bad record (its texts pass the next record)";
  return nullptr;
}

// The queries and results of n units over n_pat patterns and their records: null when they are good.
inline const char* side_units_wrong(const pgpu_unit_query* q, const pgpu_unit_result* u, size_t n, const void* recs,
                                    const uint64_t* rec_first, size_t n_pat) {
  if (n > TEXT_MAX_COUNT || n_pat > TEXT_MAX_COUNT) return TEXT_TOO_MANY;
  for (size_t i = 0; i < n; ++i) {
    const pgpu_unit_query& x = q[i];
    const pgpu_unit_result& r = u[i];
    if (r.verdict > PGPU_UNIT_ALIGNED) return "bad unit (a verdict above 2)";
    if (r.strand > 1) return "bad unit (a strand above 1)";
    if (x.fwd >= n_pat) return "bad unit (fwd is no pattern)";
    if (x.rev != PGPU_UNIT_NO_SIBLING && x.rev >= n_pat) return "bad unit (rev is neither a pattern nor PGPU_UNIT_NO_SIBLING)";
    if (r.strand == 1 && x.rev == PGPU_UNIT_NO_SIBLING) return "bad unit (strand 1 without a sibling)";
    if (r.pattern != (r.strand ? x.rev : x.fwd)) return "bad unit (pattern is not the query's pattern of that strand)";
    if (r.verdict == PGPU_UNIT_HOST) continue;
    if (const char* wrong = side_record_wrong(recs, rec_first, x.fwd)) return wrong;
    if (r.strand == 1)
      if (const char* wrong = side_record_wrong(recs, rec_first, x.rev)) return wrong;
  }
  return nullptr;
}

// The stage's device block for n units.  Offsets are multiples of 256.  The three blobs are not part of it: their sizes are
// known only after the count pass.
struct SideLayout {
  size_t out;                               // per unit: the result
  size_t counts[3], first[3];               // per unit: the bytes of megs(u), pmegs(u), edges(u); their scans
  size_t scan_tmp;
  size_t total;
};
inline SideLayout side_layout(size_t n, size_t scan_tmp_bytes) {
  SideLayout L;
  BlockCarver c;
  L.out = c.take(n * sizeof(pgpu_side_result));
  for (int k = 0; k < 3; ++k) { L.counts[k] = c.take((n + 1) * sizeof(uint32_t)); L.first[k] = c.take((n + 1) * sizeof(uint64_t)); }
  L.scan_tmp = c.take(scan_tmp_bytes);
  L.total = c.at;
  return L;
}
// The outer block of pgpu_unit_sides in front of the stage's: what the plan form finds in HBM already.  Headers and
// sequences have TEXT_PAD behind them, and so have the records.
struct SideCallLayout {
  size_t q, units, recs, rec_first, hdr, hdr_first, seqs, seq_first, stage;
};
inline SideCallLayout side_call_layout(size_t n, size_t recs_len, size_t n_pat, size_t headers_len, size_t seqs_len) {
  SideCallLayout L;
  BlockCarver c;
  L.q = c.take(n * sizeof(pgpu_unit_query)); L.units = c.take(n * sizeof(pgpu_unit_result));
  L.recs = c.take(recs_len + TEXT_PAD); L.rec_first = c.take((n_pat + 1) * sizeof(uint64_t));
  L.hdr = c.take(headers_len + TEXT_PAD); L.hdr_first = c.take((n + 1) * sizeof(uint64_t));
  L.seqs = c.take(seqs_len + TEXT_PAD); L.seq_first = c.take((n_pat + 1) * sizeof(uint64_t));
  L.stage = c.at;
  return L;
}
// The three blobs in one allocation: where each begins, and the size of the whole
struct SideBlobs { size_t at[3], total; };
inline SideBlobs side_blobs(const unsigned long long total[3]) {
  SideBlobs B;
  BlockCarver c;
  for (int k = 0; k < 3; ++k) B.at[k] = c.take((size_t)total[k]);
  B.total = c.at;
  return B;
}
