// The rules of pgpu_index_candidates on the records a caller hands in (include/pintron_gpu.h): plain host code without a HIP
// call, in a header so that tests/hostcheck/cand_call_check.cpp runs the very code of the entry under the sanitizers.  The
// kernel trusts what passes here: every read it makes lies inside the record, every genomic position it derives from a
// pairing lies inside [0, length of the sequence], and its int arithmetic does not overflow.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pintron_gpu.h"

constexpr int32_t CAND_SOURCE_P = INT32_MIN;          // EF_SOURCE_START / EF_SINK_START / EF_SOURCE_LEN of the host,
constexpr int32_t CAND_SINK_P = INT32_MAX - 200;      // SRC_START / SINK_START of pgpu_meg.hip
constexpr int32_t CAND_MARK_LEN = 200;
constexpr uint32_t CAND_MAX_FACTOR_LEN = 1u << 24;
constexpr int32_t CAND_MAX_P_END = 1 << 29;           // p + l of a pairing

inline bool cand_params_ok(const pgpu_cand_params& p) { return p.min_factor_len >= 1 && p.min_factor_len <= CAND_MAX_FACTOR_LEN; }

// One record of `len` bytes (the caller has checked that it lies inside the buffer).  The fields are read with memcpy:
// the caller's buffer need not be aligned, only the record's offset in it.
inline bool cand_record_ok(const uint8_t* rec, size_t len, size_t glen) {
  if (len < 16) return false;
  uint32_t head[4];
  memcpy(head, rec, 16);
  const uint32_t nv = head[0], ne = head[1], flags = head[2];
  if (flags & (PGPU_MEG_UNAVAILABLE | PGPU_MEG_TOO_COMPLEX)) return true;       // a bare header as far as this entry reads
  if (nv > PGPU_MEG_MAX_VERTICES) return false;
  const size_t o_first = 16 + 12 * (size_t)nv, o_tgt = o_first + 2 * ((size_t)nv + 1);
  if (len < o_tgt || (size_t)ne > len - o_tgt) return false;
  for (uint32_t k = 0; k < nv; ++k) {
    int32_t v[3];
    memcpy(v, rec + 16 + 12 * (size_t)k, 12);
    const int32_t p = v[0], t = v[1], l = v[2];
    if (p == CAND_SOURCE_P || p == CAND_SINK_P) {
      if (t != p || l != CAND_MARK_LEN) return false;
      continue;
    }
    if (p < 0 || l < 0 || t < 0 || l > CAND_MAX_P_END || p > CAND_MAX_P_END - l) return false;
    if ((size_t)t > glen || (size_t)l > glen - (size_t)t) return false;
  }
  uint16_t prev = 0;
  for (uint32_t k = 0; k <= nv; ++k) {
    uint16_t f;
    memcpy(&f, rec + o_first + 2 * (size_t)k, 2);
    if (f < prev || f > ne) return false;
    prev = f;
  }
  for (uint32_t e = 0; e < ne; ++e)
    if (rec[o_tgt + e] >= nv) return false;
  return true;
}

inline bool cand_records_ok(const void* records, size_t records_len, const uint64_t* rec_first, size_t n, size_t glen) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t a = rec_first[i], b = rec_first[i + 1];
    if (b < a || b > records_len || (a & 3u)) return false;
    if (!cand_record_ok((const uint8_t*)records + a, (size_t)(b - a), glen)) return false;
  }
  return true;
}
