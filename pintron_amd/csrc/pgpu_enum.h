// The host-only rules of pgpu_index_candidate_lists (include/pintron_gpu.h): what it refuses before a HIP call -- the
// validator is pgpu_index_candidates' own (pgpu_cand.h), unchanged -- and the three-level layout of its device block.  Plain
// host code in a header, so that tests/hostcheck/enum_call_check.cpp runs the very code of the entry under the sanitizers.
#pragma once
#include "pgpu_cand.h"
#include "pgpu_layout.h"

// What the entry checks without touching the device, in the entry's order: a null pointer, the record count, the parameters,
// the records.  0: the call goes on; otherwise a line of ENUM_REFUSALS (1 is the bare PGPU_EINVAL without a message).
enum : int { ENUM_OK = 0, ENUM_NULL, ENUM_TOO_MANY, ENUM_PARAMS, ENUM_RECORDS };
inline int enum_call_refusal(const void* ctx, const void* idx, const void* records, size_t records_len, const uint64_t* rec_first,
                             size_t n, const pgpu_cand_params* params, const void* out, const void* cands, size_t cands_cap,
                             const void* exons, size_t exons_cap, const size_t* n_cands, const size_t* n_exons, size_t glen) {
  if (!ctx || !idx || !params || !n_cands || !n_exons || (n && (!rec_first || !out)) || (records_len && !records) ||
      (cands_cap && !cands) || (exons_cap && !exons))
    return ENUM_NULL;
  if (n > 0x7fffffffull) return ENUM_TOO_MANY;
  if (!cand_params_ok(*params)) return ENUM_PARAMS;
  if (!cand_records_ok(records, records_len, rec_first, n, glen)) return ENUM_RECORDS;
  return ENUM_OK;
}

// The first device block: [records | offsets | results | candidate counts (n + 1) | exon counts (n + 1) | first candidate
// (n + 1) | first exon (n + 1) | scan workspace], every part at a multiple of 256.  The records are at 0.
struct EnumLayout { size_t first, res, cnt_c, cnt_e, off_c, off_e, tmp, total; };
inline EnumLayout enum_layout(size_t rec_bytes, size_t n, size_t scan_tmp_bytes) {
  BlockCarver c{up256(rec_bytes + 4)};
  EnumLayout L;
  L.first = c.take((n + 1) * sizeof(uint64_t));
  L.res = c.take(n * sizeof(pgpu_enum_result));
  L.cnt_c = c.take((n + 1) * sizeof(uint32_t));
  L.cnt_e = c.take((n + 1) * sizeof(uint32_t));
  L.off_c = c.take((n + 1) * sizeof(uint64_t));
  L.off_e = c.take((n + 1) * sizeof(uint64_t));
  L.tmp = c.take(scan_tmp_bytes);
  L.total = c.at;
  return L;
}
// The second one, sized by the two scans: [candidates | exons]; an empty part still has an address of its own.
struct EnumOutLayout { size_t cands, exons, total; };
inline EnumOutLayout enum_out_layout(size_t n_cands, size_t n_exons) {
  BlockCarver c;
  EnumOutLayout L;
  L.cands = c.take(n_cands * sizeof(pgpu_enum_candidate));
  L.exons = c.take(n_exons * sizeof(pgpu_factor));
  L.total = c.at;
  return L;
}
// first_candidate and first_exon are 32 bits wide: the totals of a call have to fit (a record has at most 512 candidates of
// at most 64 exons each, so only a call of more than 131 071 records can fail this)
inline bool enum_totals_fit(unsigned long long n_cands, unsigned long long n_exons) {
  return n_cands <= 0xffffffffull && n_exons <= 0xffffffffull;
}
