// The candidates of an EST taken to its list of factorizations on the device, nothing leaving HBM in between.  Semantics:
// include/pintron_gpu.h (pgpu_index_factorization_lists, pgpu_pairing_plan_run_factorization_lists).
//
// One slot = one candidate at every stage, as pgpu_fact.hip has one slot per EST: query c of clean, gaps and refine is
// candidate c of the call's table.  The three stage kernels are the ones of the chained entries, launched through
// pgpu_stage_launch.h and unchanged; a candidate with nothing to do at a stage runs that stage's trivial query on a
// placeholder exon of its own (entry n_exons_total + c of every exon array), so nothing is compacted between two stages and
// the one host wait of a call is the one that sizes clean's workspace (the atomicMax of clean_query_need).  The hand-offs
// lie at kernel boundaries on the one stream; there is no other atomic and no flag polled across workgroups.
//
//   flist_owner_kernel        one thread per EST: stage 0 (no candidate, more than 64), and the EST's index into the slot of
//                             each of its candidates.
//   flist_to_clean_kernel     one thread per candidate: the clean query; what pgpu_index_clean_chains' validator refuses
//                             is code 2 in the slot; the workspace need is folded into two words.
//   flist_clean_to_select_kernel  one thread per candidate: clean's result as the slot's kept run, or code 1 (PGPU_ERANGE).
//   flist_select_kernel       THE NEW HOT PATH: one wave per EST (one wave per workgroup, striding).  Lane i holds candidate i
//                             of the EST; the list is a 64-bit mask of lanes, wave-uniform -- appends happen in candidate order
//                             and removals keep the order, so the list's order is lane order and a removal clears a bit
//                             where a list in memory would move its survivors down to their popcount.  Per append the exons
//                             of to_add are copied into LDS (64 x 16 B) and every lane whose bit is set computes
//                             res(to_add, its entry) by walking both exon runs; two ballots give the first res < 0 and the
//                             removal mask in front of it.  The -2 widening is done in place, in the clean-output exon
//                             array, by the entry's own lane (it holds the entry's address; one lane writes), and a
//                             workgroup fence stands between it and the next append's reads.  FILTER 1 and FILTER 3 run
//                             with one lane per entry: a butterfly max in FP64 for max_cov; min_gl is folded over the
//                             lanes in list order with readlane, because the reference's `min_gl == -1` test makes that
//                             minimum depend on the order.  Everything the fold decides comes from ballots and readlane.
//                             Loop bounds: appends <= 64 per EST; a compare walks <= 64 + 64 exons (the search along the
//                             longer list, then both lists together); the inner cfr_type walk <= 64 exons of the longer
//                             list.  LDS: 1 024 bytes (to_add).  No scratch, no spilled VGPR
//                             (tests/test_flists_resources.py).
//   flist_select_to_gaps_kernel   one thread per candidate: the gaps query of an entry left, once gaps_query_ok has passed.
//   flist_gaps_verdict_kernel one thread per EST: HOST at stage 3, the entries check_gap_errors drops, EMPTY, and
//                             max_number_of_factorizations.
//   flist_gaps_to_refine_kernel   one thread per candidate: the exons gaps kept, moved down, and the chain query.
//   flist_gather_kernel<false> one thread per EST: HOST at stage 4 or DONE, and the two counts for the scans;
//   flist_gather_kernel<true>  the factorizations, exons and step bytes, compact: EST order, then list order.
//
// FP64 and contraction: the three operations of FILTER 1 that feed a comparison are written with __ddiv_rn, __dsub_rn and
// __dmul_rn, which the compiler never fuses, and the file states `#pragma clang fp contract(off)` besides, so no
// product-and-compare of this file can become an FMA whatever the build's flags are.
#pragma clang fp contract(off)
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_gaps.h"
#include "pgpu_stage_launch.h"
#include "pgpu_stage_drive.h"
#include "pgpu_flists.h"

namespace {

constexpr uint32_t FLIST_PENDING = 3u;      // outcome while the EST is on its way: never leaves the device

__device__ __forceinline__ pgpu_factor placeholder_exon() { pgpu_factor f; f.EST_start = f.EST_end = f.GEN_start = f.GEN_end = -1; return f; }
__device__ __forceinline__ void settle(pgpu_flist_result& r, uint32_t outcome, uint32_t stage, uint32_t detail) {
  r.outcome = (uint8_t)outcome; r.stage = (uint8_t)stage; r.detail = (uint16_t)detail;
}
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// the EST of record r: a query of the index form, or a plan's pattern
struct Records {
  const pgpu_flist_query* q; const unsigned long long* pat_off; const pgpu_enum_result* er;
  __device__ pgpu_flist_query get(uint32_t r, uint32_t& kind) const {
    if (q) { kind = PGPU_ENUM_LISTS; return q[r]; }
    const unsigned long long a = pat_off[r], b = pat_off[r + 1];
    const pgpu_enum_result e = er[r];
    pgpu_flist_query x;
    x.est_off = a; x.est_len = (uint32_t)(b - a); x.first_candidate = e.first_candidate; x.n_candidates = e.n_candidates; x.reserved = 0;
    kind = e.kind;
    return x;
  }
};

__global__ __launch_bounds__(256)
void flist_owner_kernel(Records recs, uint32_t n, uint32_t n_cands, FlistSlot* __restrict__ slot, pgpu_flist_result* __restrict__ res) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint32_t kind;
  const pgpu_flist_query x = recs.get(r, kind);
  pgpu_flist_result R;
  R.outcome = (uint8_t)FLIST_PENDING; R.stage = 0; R.detail = 0; R.first_fact = 0; R.n_facts = 0; R.n_cleaned = 0; R.n_listed = 0; R.n_filtered = 0;
  if (kind != PGPU_ENUM_LISTS) settle(R, PGPU_FACT_HOST, 0, kind);
  else if (x.n_candidates == 0) settle(R, PGPU_FACT_EMPTY, 0, 0);
  else if (x.n_candidates > PGPU_FLIST_MAX_CANDIDATES) settle(R, PGPU_FACT_HOST, 0, PGPU_FLIST_CAP_CANDIDATES);
  else if (x.n_candidates > n_cands || x.first_candidate > n_cands - x.n_candidates) settle(R, PGPU_FACT_HOST, 1, 2);   // (a guard: neither form hands such a range in)
  else
    for (uint32_t c = 0; c < x.n_candidates; ++c) slot[x.first_candidate + c].rec = r;
  res[r] = R;
}

__global__ __launch_bounds__(256)
void flist_to_clean_kernel(Records recs, const pgpu_enum_candidate* __restrict__ cands, uint32_t n_cands, uint32_t n_exons_total,
                           uint32_t tlen, double complexity_threshold, pgpu_factor* __restrict__ ex_in,
                           pgpu_factor* __restrict__ ex_clean, pgpu_clean_query* __restrict__ cq, FlistSlot* __restrict__ slot,
                           uint32_t* __restrict__ need) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cands) return;
  FlistSlot s = slot[c];                     // rec: the owner kernel's, or the memset's FLIST_NO_RECORD
  s.first = 0; s.n = 0; s.code = 0; s.state = 0; s.n_merged = 0; s.total_edit = 0;
  const uint32_t own = n_exons_total + c;
  ex_in[own] = placeholder_exon(); ex_clean[own] = placeholder_exon();
  pgpu_clean_query q;
  q.est_off = 0; q.est_len = 1; q.first_exon = own; q.n_exons = 1; q.reserved = 0; q.complexity_threshold = complexity_threshold;   // verdict 1 at step 1
  if (s.rec != FLIST_NO_RECORD) {
    uint32_t kind;
    const pgpu_flist_query x = recs.get(s.rec, kind);
    const pgpu_enum_candidate k = cands[c];
    q.est_off = x.est_off; q.est_len = x.est_len;
    if (k.n_exons == 0 || k.n_exons > n_exons_total || k.first_exon > n_exons_total - k.n_exons) s.code = 2;      // (a guard)
    else {
      const pgpu_factor* const ex = ex_in + k.first_exon;
      bool ok = true;
      for (uint32_t e = 0; e < k.n_exons && ok; ++e) ok = factor_ok(ex[e], x.est_len, tlen);
      size_t dirs = CLEAN_WS_DIRS_MIN, rows = CLEAN_WS_ROWS_MIN;
      if (ok) ok = clean_query_need(ex, k.n_exons, x.est_len, tlen, dirs, rows);
      if (!ok) s.code = 2;
      else {
        q.first_exon = k.first_exon; q.n_exons = k.n_exons;
        if (dirs > CLEAN_WS_DIRS_MIN) atomicMax(need, (uint32_t)dirs);
        if (rows > CLEAN_WS_ROWS_MIN) atomicMax(need + 1, (uint32_t)rows);
      }
    }
  }
  cq[c] = q;
  slot[c] = s;
}

__global__ __launch_bounds__(256)
void flist_clean_to_select_kernel(const pgpu_clean_query* __restrict__ cq, const pgpu_clean_result* __restrict__ cr, uint32_t n_cands,
                                  FlistSlot* __restrict__ slot) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cands) return;
  FlistSlot s = slot[c];
  if (s.rec == FLIST_NO_RECORD || s.code) return;
  const pgpu_clean_result a = cr[c];
  if (a.status != PGPU_OK) s.code = 1;
  else if (a.verdict == 0) { s.first = cq[c].first_exon + a.first_kept; s.n = (uint16_t)a.n_kept; }
  slot[c] = s;
}

// ---- add_if_not_exists' comparison (src/list.c:320-483, src/est-factorizations.c:1159-1259): l1 is the longer list
struct ExRun { const pgpu_factor* p; int n; };

__device__ int relaxed_factor_compare(const pgpu_factor p1, const pgpu_factor p2, int cfr_type, int allowed, const ExRun l1) {
  if (p1.GEN_start < p2.GEN_start && p1.GEN_end < p2.GEN_start) return 1;
  if (p2.GEN_start < p1.GEN_start && p2.GEN_end < p1.GEN_start) return 1;
  const int max_unconf = 20;
  if (cfr_type == 0) {
    if (iabs(p1.GEN_end - p2.GEN_end) <= allowed && iabs(p1.GEN_start - p2.GEN_start) <= allowed) return 0;
  }
  if (iabs(cfr_type) == 2) {
    if (iabs(p1.GEN_end - p2.GEN_end) <= allowed) {
      if (cfr_type == 2) {
        const int d = p1.GEN_start - p2.GEN_start;
        if (d > max_unconf) return 1;
        if (d > 0) {
          int tot = 0;
          for (int k = 0; k < l1.n; ++k) {                       // <= 64
            const pgpu_factor f = l1.p[k];
            if (p1.GEN_start == f.GEN_start) break;
            tot += f.GEN_end - f.GEN_start + 1;
          }
          if (iabs(d - tot) < 10) return 1;
        }
      }
      return 0;
    }
  }
  if (iabs(cfr_type) == 1) {
    if (iabs(p1.GEN_start - p2.GEN_start) <= allowed) {
      if (cfr_type == 1) {
        const int d = p2.GEN_end - p1.GEN_end;
        if (d > max_unconf) return 1;
        if (d > 0) {
          int tot = 0;
          for (int k = l1.n - 1; k >= 0; --k) {                  // <= 64
            const pgpu_factor f = l1.p[k];
            if (p1.GEN_start == f.GEN_start) break;
            tot += f.GEN_end - f.GEN_start + 1;
          }
          if (iabs(d - tot) < 20) return 1;
        }
      }
      return 0;
    }
  }
  return 1;
}

// relaxed_list_contained(a = to_add, b = the entry): 0 different, -1 a in b, 1 b in a, -2 equal.  allowed >= 0 (the
// parameters are checked), so the reference's `allowed_diff == -1` branches are not restated.
__device__ int relaxed_list_contained(const ExRun a, const ExRun b, int allowed) {
  if (a.n == b.n) {
    if (a.n == 1) return 0;
    for (int k = 0; k < a.n; ++k) {
      const int type = k == 0 ? -2 : (k == a.n - 1 ? -1 : 0);
      if (relaxed_factor_compare(a.p[k], b.p[k], type, allowed, a) != 0) return 0;
    }
    return -2;
  }
  if (a.n == 1 || b.n == 1) return 0;
  const bool a_longer = a.n > b.n;
  const ExRun lng = a_longer ? a : b, sht = a_longer ? b : a;
  int il = 0, is = 0, type = -2, count_long = 1;
  bool found = false;
  while (il < lng.n && !found) {
    if (relaxed_factor_compare(lng.p[il], sht.p[is], type, allowed, lng) == 0) { found = true; ++is; }
    else ++count_long;
    ++il;
    if (type == -2) type = 2;
  }
  if (!found) return 0;
  int count_factors = 1;
  bool stop = false;
  while (il < lng.n && is < sht.n && !stop) {
    type = (count_factors + 1 == sht.n) ? ((count_long + 1 == lng.n) ? -1 : 1) : 0;
    if (relaxed_factor_compare(lng.p[il], sht.p[is], type, allowed, lng) == 0) { ++il; ++is; }
    else stop = true;
    ++count_factors; ++count_long;
  }
  if (stop) return 0;
  return count_factors == sht.n ? (a_longer ? 1 : -1) : 0;
}

__device__ int flist_res(const ExRun a, const ExRun b, int allowed) {
  if (a.n == 1 && b.n == 1) {                                    // :2053-2066
    const pgpu_factor h1 = a.p[0], h2 = b.p[0];
    if (h1.GEN_start == h2.GEN_start && h1.GEN_end == h2.GEN_end) return -2;
    if (h1.GEN_start >= h2.GEN_start && h1.GEN_end <= h2.GEN_end) return -1;
    if (h1.GEN_start <= h2.GEN_start && h1.GEN_end >= h2.GEN_end) return 1;
    return 0;
  }
  return relaxed_list_contained(a, b, allowed);
}

__device__ __forceinline__ pgpu_flist_result selected(uint32_t outcome, uint32_t stage, uint32_t detail, uint32_t n_cleaned,
                                                      uint32_t n_listed, uint32_t n_filtered) {
  pgpu_flist_result r;
  r.outcome = (uint8_t)outcome; r.stage = (uint8_t)stage; r.detail = (uint16_t)detail; r.first_fact = 0; r.n_facts = 0;
  r.n_cleaned = (uint16_t)n_cleaned; r.n_listed = (uint16_t)n_listed; r.n_filtered = (uint16_t)n_filtered;
  return r;
}

__device__ __forceinline__ double wave_max_f64(double v) {
  for (int o = 32; o; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = v < w ? w : v; }
  return v;
}

__global__ __launch_bounds__(64)
void flist_select_kernel(Records recs, uint32_t n, pgpu_factor* ex_clean, FlistSlot* slot, pgpu_flist_result* __restrict__ res,
                         double max_coverage_diff, int allowed, int max_gaplength_diff) {
  __shared__ pgpu_factor add[64];
  static_assert(PGPU_CLEAN_MAX_EXONS <= 64 && PGPU_FLIST_MAX_CANDIDATES <= 64,
                "a kept run of clean_kernel fits `add` (clean refuses longer lists), and a candidate has a lane");
  const int lane = (int)threadIdx.x;
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    if (res[r].outcome != FLIST_PENDING) continue;               // uniform
    uint32_t kind;
    const pgpu_flist_query x = recs.get(r, kind);
    const int m = (int)x.n_candidates;                           // 1 .. 64
    const bool mine = lane < m;
    uint32_t s_first = 0, s_code = 0, s_state = 0;
    int s_n = 0;
    if (mine) { const FlistSlot s = slot[x.first_candidate + lane]; s_first = s.first; s_n = s.n; s_code = s.code; }
    // ---- stage 1: a cap or a refused input of any candidate
    const unsigned long long bad = __ballot(mine && s_code != 0);
    if (bad) {
      const int code = __shfl((int)s_code, __builtin_ctzll(bad), 64);
      if (lane == 0) res[r] = selected(PGPU_FACT_HOST, 1, (uint32_t)code, 0, 0, 0);
      continue;
    }
    const unsigned long long kept = __ballot(mine && s_n != 0);
    const uint32_t n_cleaned = (uint32_t)__popcll(kept);
    if (!kept) {
      if (lane == 0) res[r] = selected(PGPU_FACT_EMPTY, 1, 0, 0, 0, 0);
      continue;
    }
    // ---- add_if_not_exists, folded in candidate order
    const ExRun my = { ex_clean + s_first, s_n };
    unsigned long long list = 0;
    for (unsigned long long todo = kept; todo; todo &= todo - 1) {   // <= 64 appends
      const int j = __builtin_ctzll(todo);
      const int nj = __shfl(s_n, j, 64);
      const uint32_t fj = (uint32_t)__shfl((int)s_first, j, 64);
      __syncthreads();
      if (lane < nj) add[lane] = ex_clean[fj + lane];
      __syncthreads();
      const ExRun to_add = { add, nj };
      int rs = 0;
      if (list >> lane & 1ull) rs = flist_res(to_add, my, allowed);
      const unsigned long long neg = __ballot(rs < 0);
      unsigned long long one = __ballot(rs == 1);
      if (neg) {
        const int stop = __builtin_ctzll(neg);
        one &= (1ull << stop) - 1ull;
        if (lane == stop && rs == -2) {                          // the widening, in place
          const pgpu_factor h1 = add[0], t1 = add[nj - 1];
          pgpu_factor h2 = my.p[0];
          if (h1.EST_start < h2.EST_start) { h2.EST_start = h1.EST_start; h2.GEN_start = h1.GEN_start; ex_clean[s_first] = h2; s_state |= FLIST_HEAD; }
          pgpu_factor t2 = my.p[my.n - 1];
          if (t1.EST_end > t2.EST_end) { t2.EST_end = t1.EST_end; t2.GEN_end = t1.GEN_end; ex_clean[s_first + my.n - 1] = t2; s_state |= FLIST_TAIL; }
        }
        __threadfence_block();
      } else {
        list |= 1ull << j;
      }
      list &= ~one;
    }
    const uint32_t n_listed = (uint32_t)__popcll(list);
    // ---- FILTER 1 (:278-331)
    bool alive = (list >> lane & 1ull) != 0;
    const int len = (int)x.est_len;
    double cov = -1.0;
    int g = 0;
    if (alive) {
      const pgpu_factor h = my.p[0], t = my.p[my.n - 1];
      const bool src_sink = my.n == 1 && (h.EST_start < 0 || h.EST_start >= len);
      if (!src_sink) {
        const int cover = len - (h.EST_start + (len - t.EST_end - 1));
        cov = __ddiv_rn((double)cover, (double)len);
      }
      int prev_end = h.EST_end;
      for (int k = 1; k < my.n; ++k) { const pgpu_factor f = my.p[k]; g += f.EST_start - prev_end - 1; prev_end = f.EST_end; }
    }
    const double max_cov = wave_max_f64(alive && cov != -1.0 ? cov : 0.0);     // `max_cov < cov` from 0.0
    if (alive) {
      const double d = __dsub_rn(max_cov, cov);
      if (cov == -1.0 || d > max_coverage_diff) alive = false;
      else if (__dmul_rn(d, (double)len) > 100.0) alive = false;
    }
    list = __ballot(alive);
    // ---- FILTER 3 (:376-414): min_gl in list order, its -1 test included
    int min_gl = -1;
    for (unsigned long long todo = list; todo; todo &= todo - 1) {
      const int gk = __shfl(g, __builtin_ctzll(todo), 64);
      if (min_gl == -1 || min_gl > gk) min_gl = gk;
    }
    if (alive && max_gaplength_diff != -1 && g - min_gl > max_gaplength_diff) alive = false;
    list = __ballot(alive);
    const uint32_t n_filtered = (uint32_t)__popcll(list);
    if (mine) slot[x.first_candidate + lane].state = (uint8_t)(s_state | (alive ? FLIST_ALIVE : 0u));
    if (lane == 0)                                               // (EMPTY here is a guard: neither filter can empty the list)
      res[r] = selected(list ? FLIST_PENDING : PGPU_FACT_EMPTY, list ? 0 : 2, 0, n_cleaned, n_listed, n_filtered);
  }
}

__global__ __launch_bounds__(256)
void flist_select_to_gaps_kernel(Records recs, const pgpu_flist_result* __restrict__ res, uint32_t n_cands, uint32_t n_exons_total,
                                 const pgpu_factor* __restrict__ ex_clean, pgpu_gaps_query* __restrict__ gq, FlistSlot* __restrict__ slot) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cands) return;
  FlistSlot s = slot[c];
  pgpu_gaps_query q;
  q.est_off = 0; q.est_len = 1; q.first_exon = n_exons_total + c; q.n_exons = 1; q.reserved = 0;      // verdict 0, no DP
  if (s.rec != FLIST_NO_RECORD && res[s.rec].outcome == FLIST_PENDING && (s.state & FLIST_ALIVE)) {
    uint32_t kind;
    const pgpu_flist_query x = recs.get(s.rec, kind);
    pgpu_gaps_query g = q;
    g.est_off = x.est_off; g.est_len = x.est_len; g.first_exon = s.first; g.n_exons = s.n;
    if (!gaps_query_ok(g, ex_clean + g.first_exon)) { s.state |= FLIST_BAD_GAPS; slot[c] = s; }
    else q = g;
  }
  gq[c] = q;
}

__global__ __launch_bounds__(256)
void flist_gaps_verdict_kernel(Records recs, uint32_t n, const pgpu_gaps_result* __restrict__ gr, FlistSlot* __restrict__ slot,
                               pgpu_flist_result* __restrict__ res, int max_facts) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  pgpu_flist_result R = res[r];
  if (R.outcome != FLIST_PENDING) return;
  uint32_t kind;
  const pgpu_flist_query x = recs.get(r, kind);
  int left = 0;
  for (uint32_t k = 0; k < x.n_candidates; ++k) {                // <= 64; the lowest index decides
    FlistSlot s = slot[x.first_candidate + k];
    if (!(s.state & FLIST_ALIVE)) continue;
    if (s.state & FLIST_BAD_GAPS) { settle(R, PGPU_FACT_HOST, 3, 2); break; }
    const pgpu_gaps_result a = gr[x.first_candidate + k];
    if (a.status != PGPU_OK) { settle(R, PGPU_FACT_HOST, 3, 1); break; }
    if (a.verdict != 0) s.state &= (uint8_t)~FLIST_ALIVE;
    else { s.total_edit = (uint16_t)a.total_edit; ++left; }
    slot[x.first_candidate + k] = s;
  }
  if (R.outcome == FLIST_PENDING) {
    if (left == 0) settle(R, PGPU_FACT_EMPTY, 3, 1);
    else if (max_facts != 0 && left > max_facts) settle(R, PGPU_FACT_EMPTY, 3, 2);      // :438-442
  }
  res[r] = R;
}

__global__ __launch_bounds__(256)
void flist_gaps_to_refine_kernel(const pgpu_flist_result* __restrict__ res, uint32_t n_cands, uint32_t n_exons_total,
                                 const pgpu_gaps_query* __restrict__ gq, const pgpu_factor* __restrict__ ex_gaps,
                                 const uint8_t* __restrict__ gsteps, pgpu_flist_params prm, pgpu_factor* __restrict__ ex_kept,
                                 pgpu_chain_query* __restrict__ rq, FlistSlot* __restrict__ slot) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cands) return;
  FlistSlot s = slot[c];
  const pgpu_gaps_query g = gq[c];
  pgpu_chain_query q;
  q.est_off = 0; q.est_len = 1; q.first_exon = n_exons_total + c; q.n_exons = 1; q.reserved = 0;      // done 0
  q.suffpref_length_on_est = prm.suffpref_length_on_est; q.suffpref_length_for_intron = prm.suffpref_length_for_intron;
  q.suffpref_length_on_gen = prm.suffpref_length_on_gen; q.min_intron_length = prm.min_intron_length;
  ex_kept[n_exons_total + c] = placeholder_exon();
  if (s.rec != FLIST_NO_RECORD && res[s.rec].outcome == FLIST_PENDING && (s.state & FLIST_ALIVE)) {
    // the exons check_gap_errors kept, moved down: the donors hold their merged ends already
    uint32_t kept = 0;
    bool ordered = true;
    pgpu_factor prev = placeholder_exon();
    for (uint32_t k = 0; k < g.n_exons; ++k) {
      if (gsteps[g.first_exon + k] & 0x80u) continue;
      const pgpu_factor f = ex_gaps[g.first_exon + k];
      if (kept && !(prev.EST_end < f.EST_start && prev.GEN_end < f.GEN_start)) ordered = false;
      ex_kept[g.first_exon + kept] = f;
      prev = f; ++kept;
    }
    if (!ordered) s.state |= FLIST_UNORDERED;
    else { q.est_off = g.est_off; q.est_len = g.est_len; q.first_exon = g.first_exon; q.n_exons = kept; s.n_merged = (uint16_t)(g.n_exons - kept); }
    slot[c] = s;
  }
  rq[c] = q;
}

template <bool WRITE>
__global__ __launch_bounds__(256)
void flist_gather_kernel(Records recs, uint32_t n, const FlistSlot* __restrict__ slot, const pgpu_chain_query* __restrict__ rq,
                         const pgpu_chain_result* __restrict__ rr, pgpu_flist_result* __restrict__ res, uint32_t* __restrict__ cnt_f,
                         uint32_t* __restrict__ cnt_e, const unsigned long long* __restrict__ first_f,
                         const unsigned long long* __restrict__ first_e, const pgpu_factor* __restrict__ ex_refined,
                         const uint8_t* __restrict__ rsteps, pgpu_flist_fact* __restrict__ facts, pgpu_factor* __restrict__ out_exons,
                         uint8_t* __restrict__ out_steps) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  pgpu_flist_result R = res[r];
  uint32_t kind;
  const pgpu_flist_query x = recs.get(r, kind);
  if (WRITE) {
    if (R.outcome != PGPU_FACT_DONE) return;
    unsigned long long f = first_f[r], e = first_e[r];
    res[r].first_fact = (uint32_t)f;
    for (uint32_t k = 0; k < x.n_candidates; ++k) {
      const uint32_t c = x.first_candidate + k;
      const FlistSlot s = slot[c];
      if (!(s.state & FLIST_ALIVE)) continue;
      const uint32_t dropped = rr[c].dropped_first ? 1u : 0u;
      const uint32_t from = rq[c].first_exon + dropped, ne = rq[c].n_exons - dropped;
      pgpu_flist_fact F;
      F.first_exon = (uint32_t)e; F.n_exons = (uint16_t)ne; F.n_merged = s.n_merged; F.candidate = c; F.total_edit = s.total_edit;
      F.flags = (uint16_t)((dropped ? PGPU_FLIST_DROPPED_FIRST : 0u) | ((s.state & FLIST_HEAD) ? PGPU_FLIST_HEAD_WIDENED : 0u) |
                           ((s.state & FLIST_TAIL) ? PGPU_FLIST_TAIL_WIDENED : 0u));
      facts[f++] = F;
      for (uint32_t i = 0; i < ne; ++i) {
        out_exons[e + i] = ex_refined[from + i];
        out_steps[e + i] = (i == 0 && !dropped) ? (uint8_t)0 : rsteps[from + i];      // chain_kernel writes no byte for a first exon
      }
      e += ne;
    }
    return;
  }
  uint32_t nf = 0, ne = 0;
  if (R.outcome == FLIST_PENDING) {
    for (uint32_t k = 0; k < x.n_candidates; ++k) {              // the lowest index decides
      const uint32_t c = x.first_candidate + k;
      const FlistSlot s = slot[c];
      if (!(s.state & FLIST_ALIVE)) continue;
      if (s.state & FLIST_UNORDERED) { settle(R, PGPU_FACT_HOST, 4, 2); break; }
      const pgpu_chain_result a = rr[c];
      if (a.status != PGPU_OK) { settle(R, PGPU_FACT_HOST, 4, 1); break; }
      ++nf; ne += rq[c].n_exons - (a.dropped_first ? 1u : 0u);
    }
    if (R.outcome == FLIST_PENDING) { settle(R, PGPU_FACT_DONE, 4, 0); R.n_facts = (uint16_t)nf; }
    else { nf = 0; ne = 0; }
    res[r] = R;
  }
  cnt_f[r] = nf; cnt_e[r] = ne;
}

thread_local double t_flist_ms = 0.0;

}  // namespace

hipError_t pgpu_flist_drive(pgpu_ctx* ctx, pgpu_flist_job& d, const pgpu_flist_params& prm) {
  const uint32_t n = d.n, C = d.n_cands, E = d.n_exons_total;
  const FlistLayout L = flist_layout(n, C, E, pgpu_scan_tmp_bytes((size_t)n + 1));
  uint8_t* const B = d.block;
  hipStream_t st = pgpu_ctx_stream(ctx);
  pgpu_factor* const ex_in = (pgpu_factor*)(B + L.ex_in);
  pgpu_factor* const ex_clean = (pgpu_factor*)(B + L.ex_clean);
  pgpu_factor* const ex_gaps = (pgpu_factor*)(B + L.ex_gaps);
  pgpu_factor* const ex_kept = (pgpu_factor*)(B + L.ex_kept);
  pgpu_factor* const ex_refined = (pgpu_factor*)(B + L.ex_refined);
  pgpu_clean_query* const cq = (pgpu_clean_query*)(B + L.cq);
  pgpu_clean_result* const cr = (pgpu_clean_result*)(B + L.cr);
  pgpu_gaps_query* const gq = (pgpu_gaps_query*)(B + L.gq);
  pgpu_gaps_result* const gr = (pgpu_gaps_result*)(B + L.gr);
  pgpu_chain_query* const rq = (pgpu_chain_query*)(B + L.rq);
  pgpu_chain_result* const rr = (pgpu_chain_result*)(B + L.rr);
  FlistSlot* const slot = (FlistSlot*)(B + L.slot);
  pgpu_flist_result* const res = (pgpu_flist_result*)(B + L.res);
  uint32_t* const need = (uint32_t*)(B + L.need);                  // ws_dirs, ws_rows, clean's `undersized` flag
  uint32_t* const cnt_f = (uint32_t*)(B + L.cnt_f);
  uint32_t* const cnt_e = (uint32_t*)(B + L.cnt_e);
  unsigned long long* const first_f = (unsigned long long*)(B + L.first_f);
  unsigned long long* const first_e = (unsigned long long*)(B + L.first_e);
  pgpu_flist_fact* const facts = (pgpu_flist_fact*)(B + L.facts);
  const Records recs = { d.q, d.pat_off, d.enum_res };
  const dim3 grid_r((n + 255) / 256), grid_c((C + 255) / 256 ? (C + 255) / 256 : 1), blk(256);
  d.total_facts = 0; d.total_exons = 0; d.undersized = 0;

  DRIVE(drive_record(d.ev, 0, st));
  const uint32_t need0[3] = { CLEAN_WS_DIRS_MIN, CLEAN_WS_ROWS_MIN, 0 };
  DRIVE(hipMemcpyAsync(need, need0, sizeof need0, hipMemcpyHostToDevice, st));
  if (E && d.cand_exons != ex_in) DRIVE(hipMemcpyAsync(ex_in, d.cand_exons, (size_t)E * sizeof(pgpu_factor), hipMemcpyDeviceToDevice, st));
  if (E) DRIVE(hipMemcpyAsync(ex_clean, ex_in, (size_t)E * sizeof(pgpu_factor), hipMemcpyDeviceToDevice, st));
  DRIVE(hipMemsetAsync(slot, 0xff, (C ? C : 1) * sizeof(FlistSlot), st));          // rec = FLIST_NO_RECORD
  hipLaunchKernelGGL(flist_owner_kernel, grid_r, blk, 0, st, recs, n, C, slot, res);
  hipLaunchKernelGGL(flist_to_clean_kernel, grid_c, blk, 0, st, recs, d.cands, C, E, d.tlen, prm.complexity_threshold, ex_in, ex_clean,
                     cq, slot, need);
  // the one host wait inside the call: what the end-exon alignments of this call need of a wave's workspace
  uint32_t sized[2] = { 0, 0 };
  DRIVE(hipMemcpyAsync(sized, need, sizeof sized, hipMemcpyDeviceToHost, st));
  DRIVE(pgpu_ctx_wait(ctx));
  DRIVE(hipGetLastError());
  const size_t ws_dirs = sized[0], ws_rows = sized[1];
  size_t waves_clean = 0, ws_wave_clean = 0, waves = 0, waves_sel = 0, cus = 0;
  DRIVE(pgpu_clean_grid(C ? C : 1, ws_dirs, ws_rows, waves_clean, ws_wave_clean));
  DRIVE(chained_waves(C ? C : 1, waves, cus));
  DRIVE(chained_waves(n, waves_sel, cus));
  // clean's and refine's workspaces are never live together: one block for both
  const size_t ws_clean = waves_clean * ws_wave_clean, ws_chain = waves * pgpu_chain_ws_wave();
  uint8_t* const ws = (uint8_t*)d.ws_alloc(d.ws_user, ws_clean > ws_chain ? ws_clean : ws_chain);
  if (!ws) return hipErrorOutOfMemory;

  DRIVE(drive_record(d.ev, 2, st));
  if (C) pgpu_clean_launch(d.T, d.tlen, d.ests, ex_in, cq, C, ws, ws_dirs, ws_rows, waves_clean, ex_clean, B + L.marks, cr, need + 2, st);
  DRIVE(drive_record(d.ev, 3, st));
  hipLaunchKernelGGL(flist_clean_to_select_kernel, grid_c, blk, 0, st, cq, cr, C, slot);
  DRIVE(drive_record(d.ev, 4, st));
  hipLaunchKernelGGL(flist_select_kernel, dim3((uint32_t)waves_sel), dim3(64), 0, st, recs, n, ex_clean, slot, res, prm.max_coverage_diff,
                     prm.max_site_difference, prm.max_gaplength_diff);
  DRIVE(drive_record(d.ev, 5, st));
  hipLaunchKernelGGL(flist_select_to_gaps_kernel, grid_c, blk, 0, st, recs, res, C, E, ex_clean, gq, slot);
  DRIVE(drive_record(d.ev, 6, st));
  if (d.given_gaps) {
    if (C) DRIVE(hipMemcpyAsync(gr, d.given_gaps->results, (size_t)C * sizeof *gr, hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(ex_gaps, d.given_gaps->exons, ((size_t)E + C) * sizeof(pgpu_factor), hipMemcpyHostToDevice, st));
    DRIVE(hipMemcpyAsync(B + L.gsteps, d.given_gaps->steps, (size_t)E + C, hipMemcpyHostToDevice, st));
  } else if (C) {
    pgpu_gaps_launch(d.T, d.ests, ex_clean, gq, C, waves, ex_gaps, B + L.gsteps, gr, st);
  }
  DRIVE(drive_record(d.ev, 7, st));
  hipLaunchKernelGGL(flist_gaps_verdict_kernel, grid_r, blk, 0, st, recs, n, gr, slot, res, prm.max_number_of_factorizations);
  hipLaunchKernelGGL(flist_gaps_to_refine_kernel, grid_c, blk, 0, st, res, C, E, gq, ex_gaps, B + L.gsteps, prm, ex_kept, rq, slot);
  DRIVE(drive_record(d.ev, 8, st));
  if (C) pgpu_chain_launch(d.T, d.tlen, d.ests, ex_kept, rq, C, ws, waves, ex_refined, B + L.rsteps, rr, st);
  DRIVE(drive_record(d.ev, 9, st));
  hipLaunchKernelGGL(flist_gather_kernel<false>, grid_r, blk, 0, st, recs, n, slot, rq, rr, res, cnt_f, cnt_e,
                     (const unsigned long long*)nullptr, (const unsigned long long*)nullptr, (const pgpu_factor*)nullptr,
                     (const uint8_t*)nullptr, (pgpu_flist_fact*)nullptr, (pgpu_factor*)nullptr, (uint8_t*)nullptr);
  DRIVE(drive_scan(cnt_f, first_f, n, B + L.scan_tmp, st));
  DRIVE(drive_scan(cnt_e, first_e, n, B + L.scan_tmp, st));
  hipLaunchKernelGGL(flist_gather_kernel<true>, grid_r, blk, 0, st, recs, n, slot, rq, rr, res, (uint32_t*)nullptr, (uint32_t*)nullptr,
                     first_f, first_e, ex_refined, B + L.rsteps, facts, (pgpu_factor*)(B + L.out_exons), B + L.out_steps);
  DRIVE(drive_record(d.ev, 1, st));
  DRIVE(hipMemcpyAsync(&d.total_facts, first_f + n, sizeof d.total_facts, hipMemcpyDeviceToHost, st));
  DRIVE(hipMemcpyAsync(&d.total_exons, first_e + n, sizeof d.total_exons, hipMemcpyDeviceToHost, st));
  DRIVE(hipMemcpyAsync(&d.undersized, need + 2, sizeof d.undersized, hipMemcpyDeviceToHost, st));
  DRIVE(pgpu_ctx_wait(ctx));
  return hipGetLastError();
}

extern "C" double pgpu_index_factorization_lists_kernel_ms(void) { return t_flist_ms; }

static int flist_index_call(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len, const pgpu_enum_candidate* cands,
                            size_t n_cands_total, const pgpu_factor* exons, size_t n_exons_total, const pgpu_flist_query* q, size_t n,
                            const pgpu_flist_params* params, pgpu_flist_result* out, pgpu_flist_fact* facts, size_t facts_cap,
                            pgpu_factor* out_exons, uint8_t* out_steps, size_t exons_cap, size_t* n_facts, size_t* n_exons,
                            const pgpu_flist_job::Given* given) {
  t_flist_ms = 0.0;      // a refused call has no kernel time either (include/pintron_gpu.h: "the last call")
  static_assert(sizeof(pgpu_flist_query) == 24 && sizeof(pgpu_flist_params) == 48 && sizeof(pgpu_flist_result) == 16 &&
                sizeof(pgpu_flist_fact) == 16, "ABI layout");
  NamedExons cand_named, exon_named;
  cand_named.p = (uint8_t*)calloc(n_cands_total && n_cands_total <= 0x7fffffffull ? n_cands_total : 1, 1);
  exon_named.p = (uint8_t*)calloc(n_exons_total && n_exons_total <= 0x7fffffffull ? n_exons_total : 1, 1);
  if (ctx && (!cand_named.p || !exon_named.p))
    return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "no memory for the tables of the candidates and exons the queries name");
  switch (flist_call_refusal(ctx, idx, ests, ests_len, cands, n_cands_total, exons, n_exons_total, q, n, params, out, facts, facts_cap,
                             out_exons, out_steps, exons_cap, n_facts, n_exons, cand_named.p, exon_named.p)) {
    case FLIST_OK: break;
    case FLIST_NULL: return PGPU_EINVAL;
    case FLIST_TOO_MANY: return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 queries, candidates or exons in one call");
    case FLIST_PARAMS:
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad factorization-list parameters (a suffpref length, max_site_difference or "
                                             "max_number_of_factorizations outside [0, 2^24], max_coverage_diff outside [0, 1], "
                                             "max_gaplength_diff < -1, or reserved != 0)");
    default:
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad factorization-list query (a range past its buffer, an empty EST, reserved != 0, a "
                                             "candidate without exons, a candidate two queries share, or an exon two candidates share)");
  }
  *n_facts = 0; *n_exons = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "factorization_lists");
  // the one device block: [ests + 64 | queries | candidates | the driver's block]; the workspace in a second one
  const FlistLayout L = flist_layout(n, n_cands_total, n_exons_total, pgpu_scan_tmp_bytes(n + 1));
  BlockCarver c{up256(ests_len + 64)};
  const size_t o_q = c.take(n * sizeof *q), o_c = c.take(n_cands_total * sizeof *cands), o_block = c.take(L.total);
  TRY_HIP(hipMalloc((void**)&call.d, c.at));
  TRY_HIP(call.timing_events(1));
  if (ests_len) TRY_HIP(hipMemcpyAsync(call.d, ests, ests_len, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + o_q, q, n * sizeof *q, hipMemcpyHostToDevice, call.st));
  if (n_cands_total) TRY_HIP(hipMemcpyAsync(call.d + o_c, cands, n_cands_total * sizeof *cands, hipMemcpyHostToDevice, call.st));
  pgpu_flist_job job;
  memset(&job, 0, sizeof job);
  job.T = pgpu_index_genomic(idx); job.tlen = (uint32_t)pgpu_index_length(idx); job.ests = call.d;
  job.q = (const pgpu_flist_query*)(call.d + o_q); job.cands = (const pgpu_enum_candidate*)(call.d + o_c);
  job.n = (uint32_t)n; job.n_cands = (uint32_t)n_cands_total; job.n_exons_total = (uint32_t)n_exons_total; job.block = call.d + o_block;
  job.cand_exons = (const pgpu_factor*)(job.block + L.ex_in);          // uploaded where the driver wants them
  job.ws_alloc = [](void* user, size_t bytes) -> void* {
    QueryCall* k = (QueryCall*)user;
    return hipMalloc((void**)&k->d2, bytes ? bytes : 16) == hipSuccess ? k->d2 : nullptr;
  };
  job.ws_user = &call;
  job.ev[0] = call.ev[0]; job.ev[1] = call.ev[1];
  job.given_gaps = given;
  if (n_exons_total) TRY_HIP(hipMemcpyAsync(job.block + L.ex_in, exons, n_exons_total * sizeof(pgpu_factor), hipMemcpyHostToDevice, call.st));
  TRY_HIP(pgpu_flist_drive(ctx, job, *params));
  if (job.undersized) return pgpu_clean_undersized(ctx, "factorization_lists");
  *n_facts = (size_t)job.total_facts; *n_exons = (size_t)job.total_exons;
  if (job.total_facts > facts_cap || job.total_exons > exons_cap)
    return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "factorization or exon buffer too small");
  TRY_HIP(hipMemcpyAsync(out, job.block + L.res, n * sizeof *out, hipMemcpyDeviceToHost, call.st));
  if (job.total_facts) TRY_HIP(hipMemcpyAsync(facts, job.block + L.facts, (size_t)job.total_facts * sizeof *facts, hipMemcpyDeviceToHost, call.st));
  if (job.total_exons) {
    TRY_HIP(hipMemcpyAsync(out_exons, job.block + L.out_exons, (size_t)job.total_exons * sizeof(pgpu_factor), hipMemcpyDeviceToHost, call.st));
    TRY_HIP(hipMemcpyAsync(out_steps, job.block + L.out_steps, (size_t)job.total_exons, hipMemcpyDeviceToHost, call.st));
  }
  TRY_HIP(pgpu_ctx_wait(ctx));
  call.elapsed_ms(0, &t_flist_ms);
  return PGPU_OK;
}

extern "C" int pgpu_index_factorization_lists(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                              const pgpu_enum_candidate* cands, size_t n_cands_total, const pgpu_factor* exons,
                                              size_t n_exons_total, const pgpu_flist_query* q, size_t n,
                                              const pgpu_flist_params* params, pgpu_flist_result* out, pgpu_flist_fact* facts,
                                              size_t facts_cap, pgpu_factor* out_exons, uint8_t* out_steps, size_t exons_cap,
                                              size_t* n_facts, size_t* n_exons) {
  return flist_index_call(ctx, idx, ests, ests_len, cands, n_cands_total, exons, n_exons_total, q, n, params, out, facts, facts_cap,
                          out_exons, out_steps, exons_cap, n_facts, n_exons, nullptr);
}

// The index form with gaps_kernel's three outputs given by the caller instead of computed (no part of the C-ABI's header; for
// tests/test_gpu_flists.py): gaps_results holds n_cands_total entries in candidate order, gaps_exons and gaps_steps
// n_exons_total + n_cands_total, the layout of the driver's block.  What gaps_kernel can never write -- two kept exons that
// are not strictly in order: its border loop sets a.EST_start = d.EST_end + 1 and its merging loop keeps only an exon more
// than 3 bases behind its donor on the sequence -- reaches the hand-off kernels behind it only this way: HOST at stage 4,
// detail 2.  Everything else is the entry above.
extern "C" int pgpu_flist_handoffs_probe(pgpu_ctx* ctx, const pgpu_index* idx, const char* ests, size_t ests_len,
                                         const pgpu_enum_candidate* cands, size_t n_cands_total, const pgpu_factor* exons,
                                         size_t n_exons_total, const pgpu_flist_query* q, size_t n, const pgpu_flist_params* params,
                                         pgpu_flist_result* out, pgpu_flist_fact* facts, size_t facts_cap, pgpu_factor* out_exons,
                                         uint8_t* out_steps, size_t exons_cap, size_t* n_facts, size_t* n_exons,
                                         const pgpu_gaps_result* gaps_results, const pgpu_factor* gaps_exons, const uint8_t* gaps_steps) {
  if (!gaps_results || !gaps_exons || !gaps_steps) return PGPU_EINVAL;
  const pgpu_flist_job::Given given = { gaps_results, gaps_exons, gaps_steps };
  return flist_index_call(ctx, idx, ests, ests_len, cands, n_cands_total, exons, n_exons_total, q, n, params, out, facts, facts_cap,
                          out_exons, out_steps, exons_cap, n_facts, n_exons, &given);
}
