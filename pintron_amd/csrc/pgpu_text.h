// The rules of pgpu_unit_texts and of pgpu_pairing_plan_run_texts on what a caller hands in (include/pintron_gpu.h), and
// the layout of the text stage's device block: plain host code without a HIP call, in a header so that
// tests/hostcheck/text_call_check.cpp runs the very code of the entries under the sanitizers.  Only structure is refused
// here: what the numbers of a group say is clipped per exon on the device (pgpu_text.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pintron_gpu.h"
#include "pgpu_layout.h"

constexpr size_t TEXT_MAX_COUNT = 0x7fffffffull;
constexpr char TEXT_TOO_MANY[] = "more than 2^31 - 1 units or patterns in one call";
// what lies behind the stage's own copies of headers, sequences and genomic: an aligned load of the copy loop reads up to
// 3 bytes past a stretch
constexpr size_t TEXT_PAD = 16;

// n + 1 offsets into `len` bytes: null when they ascend and none passes the length.  `bad`: what to say otherwise.
inline const char* text_offsets_wrong(const uint64_t* first, size_t n, size_t len, const char* bad) {
  for (size_t i = 0; i < n; ++i)
    if (first[i + 1] < first[i]) return bad;
  return first[n] > len ? bad : nullptr;
}
constexpr char TEXT_BAD_HDR[] = "bad header offsets (they do not ascend, or pass headers_len)";
constexpr char TEXT_BAD_SEQ[] = "bad sequence offsets (they do not ascend, or pass seqs_len)";

// The units over n_pat patterns and the blob of their groups: null when they are good.  Only ALIGNED units are looked at
// beyond their verdict.  The blob is read with memcpy: a caller's buffer may lie anywhere.
inline const char* text_units_wrong(const pgpu_unit_result* u, size_t n, size_t n_pat, const void* blob, size_t blob_len) {
  if (n > TEXT_MAX_COUNT || n_pat > TEXT_MAX_COUNT) return TEXT_TOO_MANY;
  const uint8_t* const B = (const uint8_t*)blob;
  for (size_t i = 0; i < n; ++i) {
    const pgpu_unit_result& x = u[i];
    if (x.verdict > PGPU_UNIT_ALIGNED) return "bad unit (a verdict above 2)";
    if (x.verdict != PGPU_UNIT_ALIGNED) continue;
    if (x.pattern >= n_pat) return "bad unit (pattern is no pattern)";
    if ((x.first_byte & 3) || (x.n_bytes & 3)) return "bad unit (first_byte or n_bytes is no multiple of 4)";
    if (x.first_byte > blob_len || x.n_bytes > blob_len - x.first_byte) return "bad unit (first_byte + n_bytes beyond the blob)";
    if (x.n_bytes < 8) return "bad group (shorter than its 8 bytes of header)";
    uint32_t n_fact;
    memcpy(&n_fact, B + x.first_byte + 4, 4);
    size_t at = 8;
    for (uint32_t f = 0; f < n_fact; ++f) {
      if (x.n_bytes - at < 4) return "bad group (its factorizations do not add up to n_bytes)";
      uint16_t n_exons;
      memcpy(&n_exons, B + x.first_byte + at + 2, 2);
      at += 4;
      if (x.n_bytes - at < 16 * (size_t)n_exons) return "bad group (its factorizations do not add up to n_bytes)";
      at += 16 * (size_t)n_exons;
    }
    if (at != x.n_bytes) return "bad group (its factorizations do not add up to n_bytes)";
  }
  return nullptr;
}

// The stage's device block for n units whose headers take headers_len bytes.  Offsets are multiples of 256.  The two
// blobs are not part of it: their sizes are known only after the count pass.
struct TextLayout {
  size_t hdr, hdr_first;                    // the headers + TEXT_PAD, their n + 1 offsets
  size_t out;                               // per unit: the result
  size_t raw_counts, raw_first;             // per unit: the bytes of raw(u); the scan
  size_t pests_counts, pests_first;         // the same for pests(u)
  size_t scan_tmp;
  size_t total;
};
inline TextLayout text_layout(size_t n, size_t headers_len, size_t scan_tmp_bytes) {
  TextLayout L;
  BlockCarver c;
  L.hdr = c.take(headers_len + TEXT_PAD); L.hdr_first = c.take((n + 1) * sizeof(uint64_t));
  L.out = c.take(n * sizeof(pgpu_text_result));
  L.raw_counts = c.take((n + 1) * sizeof(uint32_t)); L.raw_first = c.take((n + 1) * sizeof(uint64_t));
  L.pests_counts = c.take((n + 1) * sizeof(uint32_t)); L.pests_first = c.take((n + 1) * sizeof(uint64_t));
  L.scan_tmp = c.take(scan_tmp_bytes);
  L.total = c.at;
  return L;
}
// The outer block of pgpu_unit_texts in front of the stage's: what the plan form finds in HBM already.
struct TextCallLayout {
  size_t units, blob, seqs, seq_first, genomic, stage;
};
inline TextCallLayout text_call_layout(size_t n, size_t blob_len, size_t seqs_len, size_t n_pat, size_t genomic_len) {
  TextCallLayout L;
  BlockCarver c;
  L.units = c.take(n * sizeof(pgpu_unit_result)); L.blob = c.take(blob_len + TEXT_PAD);
  L.seqs = c.take(seqs_len + TEXT_PAD); L.seq_first = c.take((n_pat + 1) * sizeof(uint64_t));
  L.genomic = c.take(genomic_len + TEXT_PAD);
  L.stage = c.at;
  return L;
}
