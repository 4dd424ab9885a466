// One query of the tail stage (pgpu_index_tail_chains, include/pintron_gpu.h) as a wave answers it, for the kernels that
// differ only in the largest lost prefix or suffix they take: tail_kernel (pgpu_tail.hip) at R = 4 rows of the AFFIX body
// per lane, 256 EST bytes, and tail_wide_kernel (pgpu_tail_wide.hip) at R = 16, 1024.  The LDS of a wave follows from R:
// the two reversed windows of a lost prefix hold 64 * R EST bytes and (int)(1.17 * 64 * R) genomic ones, rounded up to 16.
// Every other cap is the same at every R.  Each dynamic program keeps its one call site.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"

namespace tail_stage {

constexpr uint32_t MAX_EXONS = PGPU_TAIL_MAX_EXONS;
constexpr uint32_t MAX_WINDOW = PGPU_TAIL_MAX_SMALL_WINDOW;
constexpr uint32_t MAX_SMALL_GEN = PGPU_TAIL_MAX_SMALL_GEN;
constexpr int UB_MED_EXON = PGPU_TAIL_UB_MED_EXON;
constexpr int AFFIXES_LENGTH = PGPU_TAIL_AFFIXES_LENGTH;
static_assert(MAX_EXONS == 64, "one lane per exon");
static_assert(MAX_WINDOW == 2 * 64, "lev_wave_body<2, BORDERS>: two rows of the pattern per lane");
static_assert(UB_MED_EXON <= 2 * 64, "lev_wave_body<2, ED>: the shorter string, at most the analysed exon, on the rows");

constexpr uint8_t STEP_PREFIX = 0x10, STEP_SUFFIX = 0x20, STEP_TAIL = 0x40;

// the cap of a lost window at R rows per lane, and the genomic window of a prefix of that many EST bytes
template <int R> constexpr uint32_t tail_max_affix() { return 64u * R; }
template <int R> constexpr uint32_t tail_max_affix_gen() { return ((uint32_t)(1.17 * (64 * R)) + 15u) & ~15u; }
static_assert(tail_max_affix<4>() == PGPU_TAIL_MAX_AFFIX && tail_max_affix_gen<4>() == 304, "the narrow kernel's windows");

template <int R>
struct TailLds {
  static_assert((uint32_t)(1.17 * tail_max_affix<R>()) <= tail_max_affix_gen<R>(), "the genomic window of a prefix");
  pgpu_factor ex[MAX_EXONS];                  // the query's exons as the steps leave them
  uint32_t rowmin[4 * (MAX_WINDOW + 1)];      // pre, pre_pos, suf, suf_pos of the analysis at hand
  DevResult res;                              // the answer of the DP at hand
  uint8_t steps[MAX_EXONS];
  uint8_t rev_e[tail_max_affix<R>()];         // the lost prefix's two windows, reversed
  uint8_t rev_g[tail_max_affix_gen<R>()];
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool is_a(uint8_t c) { return c == 'a' || c == 'A'; }

// detect_polyA_signal (src/detect-polya.c:73-166) with the tail exon's ends as step 1 left them; the loops as written.
// Returns polyA | polyadenil << 1.  Every lane walks the same bytes.
__device__ __forceinline__ uint32_t polyA_flags(const uint8_t* __restrict__ orig, const uint32_t el, const uint8_t* __restrict__ T,
                                                const uint32_t gl, const int est_end, const int gen_end) {
  const uint8_t* const cl = orig + (est_end + 1);
  const int cll = (int)el - est_end - 1;
  int i = 0, matches = 0;
  bool stop = false;
  while (i < cll && !stop) {
    if (is_a(cl[i])) { if (matches >= 8) stop = true; else { ++matches; ++i; } }
    else { if (matches >= 8) stop = true; else i = cll; }
  }
  bool polyadenil = false;
  if (stop) {
    i = gen_end - 39 > 0 ? gen_end - 39 : 0;
    while (i <= gen_end && !polyadenil) {
      if (is_a(T[i]) && (uint32_t)i + 6u <= gl) {        // a hexamer cut short by the sequence's end does not match
        const uint8_t c1 = T[i + 1], c2 = T[i + 2];
        const bool lower = T[i] == 'a';
        const uint8_t a = lower ? 'a' : 'A', t = lower ? 't' : 'T';
        polyadenil = (c1 == a || c1 == t) && c2 == t && T[i + 3] == a && T[i + 4] == a && T[i + 5] == a;
      }
      ++i;
    }
    i = gen_end - 9 > 0 ? gen_end - 9 : 0;
    matches = 0;
    while (i <= gen_end + 10 && stop && (uint32_t)i < gl) {
      if (matches >= 6) stop = false;
      else { if (is_a(T[i])) ++matches; else matches = 0; ++i; }
    }
    if (stop) {
      i = gen_end + 1;
      int count = 0;
      while (i <= gen_end + 10 && stop && (uint32_t)i < gl) {
        if (count >= 7) stop = false;
        else { if (is_a(T[i])) ++count; ++i; }
      }
    }
  }
  return (stop ? 1u : 0u) | (polyadenil ? 2u : 0u);
}

// The whole kernel: one wave per workgroup, a wave that has finished a query takes the next one of its stride.  Every step
// from the input, the answer to out[c] and, unless it is refused, to the exons and the step bytes of its range.  AGAIN: the
// wave takes only the queries a kernel before it over the same arrays left at PGPU_ERANGE, and leaves the others as they are.
template <int R, bool AGAIN>
__device__ __forceinline__ void tail_body(const uint8_t* __restrict__ T, const uint32_t gl, const uint8_t* __restrict__ ests,
                                          const pgpu_factor* __restrict__ exons, const pgpu_tail_query* __restrict__ queries,
                                          uint32_t n_queries, pgpu_factor* __restrict__ out_exons, uint8_t* __restrict__ out_steps,
                                          pgpu_tail_result* __restrict__ out) {
  constexpr uint32_t MAX_AFFIX = tail_max_affix<R>();
  __shared__ TailLds<R> S;
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_queries; c += gridDim.x) {
    if constexpr (AGAIN) { if (uni(out[c].status) != PGPU_ERANGE) continue; }
    const pgpu_tail_query q = queries[c];
    const uint8_t* const est = ests + q.est_off;
    const uint8_t* const orig = ests + q.orig_off;
    const uint32_t el = q.est_len, ne = q.n_exons;
    bool refused = ne > MAX_EXONS;
    __syncthreads();                                           // the query before is done with the LDS
    if (!refused && lane < ne) { S.ex[lane] = exons[q.first_exon + lane]; S.steps[lane] = 0; }
    __syncthreads();
    uint32_t added = 0, flags = 0, verdict = 0, recovered = 0;
    if (!refused) {
      // ---- step 1, correct_composition_tail: 64 bytes per ballot
      const int te = uni(S.ex[ne - 1].EST_end), tg = uni(S.ex[ne - 1].GEN_end);
      uint32_t i = (uint32_t)te + 1u, j = (uint32_t)tg + 1u;
      for (;;) {
        const bool eq = i + lane < el && j + lane < gl && orig[i + lane] == T[j + lane];
        const unsigned long long differ = ~__ballot(eq);
        const uint32_t run = differ ? (uint32_t)__builtin_ctzll(differ) : 64u;
        i += run; j += run;
        if (run < 64u) break;
      }
      added = i - ((uint32_t)te + 1u);
      __syncthreads();
      if (lane == 0 && added) { S.ex[ne - 1].EST_end = te + (int)added; S.ex[ne - 1].GEN_end = tg + (int)added; }
      __syncthreads();
      // ---- step 2, detect_polyA_signal
      flags = (uint32_t)uni((int)polyA_flags(orig, el, T, gl, te + (int)added, tg + (int)added));
      // ---- step 3, remove_invalid_factorizations
      bool invalid = false;
      if (lane < ne) {
        const pgpu_factor f = S.ex[lane];
        invalid = f.EST_start > f.EST_end || f.GEN_start > f.GEN_end;
        if (lane + 1 < ne) invalid = invalid || f.EST_end >= S.ex[lane + 1].EST_start || f.GEN_end >= S.ex[lane + 1].GEN_start;
      }
      verdict = __any(invalid) ? 1u : 0u;
    }
    if (!refused && verdict == 0) {
      // ---- step 4, recover_lost_prefixes_and_suffixes: side 0 the prefix, side 1 the suffix; both windows are taken from
      // the exons as they are now (a prefix moves the first exon's starts, a suffix the last one's ends), then both applied
      const int f_es = uni(S.ex[0].EST_start), f_gs = uni(S.ex[0].GEN_start);
      const int l_ee = uni(S.ex[ne - 1].EST_end), l_ge = uni(S.ex[ne - 1].GEN_end);
      uint32_t pre_e = 0, pre_g = 0, suf_len = 0;
      bool ask_pre = false, ask_suf = false;
      if (f_es > 0 && f_gs > 0) {
        const int flen = f_es < f_gs ? f_es : f_gs;
        const int cap = (int)((1.0 + 0.17) * (double)flen);
        pre_e = (uint32_t)(f_es < cap ? f_es : cap); pre_g = (uint32_t)(f_gs < cap ? f_gs : cap);
        ask_pre = est[f_es - 1] != T[f_gs - 1];
      }
      if (el - (uint32_t)l_ee > 1u && gl - (uint32_t)l_ge > 1u) {
        const uint32_t re = el - (uint32_t)l_ee - 1u, rg = gl - (uint32_t)l_ge - 1u;
        suf_len = re < rg ? re : rg;
        ask_suf = est[l_ee] != T[l_ge];
      }
      refused = (ask_pre && pre_e > MAX_AFFIX) || (ask_suf && suf_len > MAX_AFFIX);
      if (!refused && ask_pre) {
        for (uint32_t k = lane; k < pre_e; k += 64) S.rev_e[k] = est[(uint32_t)f_es - 1u - k];
        for (uint32_t k = lane; k < pre_g; k += 64) S.rev_g[k] = T[(uint32_t)f_gs - 1u - k];
      }
      uint32_t pre_cut_e = 0, pre_cut_g = 0, suf_cut_e = 0, suf_cut_g = 0;
      for (int side = 0; side < 2 && !refused; ++side) {
        if (!(side ? ask_suf : ask_pre)) continue;
        DevJob job;
        job.a = side ? est + l_ee : (const uint8_t*)S.rev_e; job.la = side ? suf_len : pre_e;
        job.b = side ? T + l_ge : (const uint8_t*)S.rev_g; job.lb = side ? suf_len : pre_g;
        job.p0 = job.p1 = job.p2 = job.tail = 0;
        job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = R;
        __syncthreads();                                       // the reversed windows; the answer before has been read
        lev_wave_body<R, MODE_AFFIX>(job, &S.res, nullptr, lane);
        __syncthreads();                                       // lane 0's answer, for every lane
        if (uni(S.res.v[0])) {
          const uint32_t ce = (uint32_t)uni(S.res.v[1]), cg = (uint32_t)uni(S.res.v[2]);
          if (side) { suf_cut_e = ce; suf_cut_g = cg; } else { pre_cut_e = ce; pre_cut_g = cg; }
          recovered |= 1u << side;
        }
      }
      if (!refused && lane == 0) {
        if (recovered & 1u) { S.ex[0].EST_start = f_es - (int)pre_cut_e; S.ex[0].GEN_start = f_gs - (int)pre_cut_g; S.steps[0] |= STEP_PREFIX; }
        if (recovered & 2u) { S.ex[ne - 1].EST_end = l_ee + (int)suf_cut_e; S.ex[ne - 1].GEN_end = l_ge + (int)suf_cut_g; S.steps[ne - 1] |= STEP_SUFFIX; }
      }
      __syncthreads();
      // ---- step 5, remove_false_small_exons (:1095-1125) with analyze_possibly_small_exon (:960-1093) in its loop
      int prev = -1, curr = -1, next = 0;
      bool removed = false;
      while (!refused) {
        if (!removed) { prev = curr; curr = next; next = (uint32_t)next + 1u < ne ? next + 1 : -1; }
        removed = false;
        if (next < 0) break;
        if (prev < 0) continue;
        const int p_es = uni(S.ex[prev].EST_start), p_ee = uni(S.ex[prev].EST_end), p_gs = uni(S.ex[prev].GEN_start), p_ge = uni(S.ex[prev].GEN_end);
        const int c_es = uni(S.ex[curr].EST_start), c_ee = uni(S.ex[curr].EST_end), c_gs = uni(S.ex[curr].GEN_start), c_ge = uni(S.ex[curr].GEN_end);
        const int n_es = uni(S.ex[next].EST_start), n_ee = uni(S.ex[next].EST_end), n_gs = uni(S.ex[next].GEN_start), n_ge = uni(S.ex[next].GEN_end);
        const int elen = c_ee + 1 - c_es, glen = c_ge + 1 - c_gs;
        if (elen > UB_MED_EXON) continue;
        uint32_t outcome = 1;
        if (p_ge < c_gs && c_ge < n_gs) {                      // (else: an earlier merge with off_t1 > off_t2 lost the order)
          const int estart = p_es + 1 > p_ee + 1 - AFFIXES_LENGTH ? p_es + 1 : p_ee + 1 - AFFIXES_LENGTH;
          const int eend = n_ee < n_es + AFFIXES_LENGTH ? n_ee : n_es + AFFIXES_LENGTH;
          const int epreflen = p_ee + 1 - estart, esufflen = eend - n_es, allelen = eend - estart;
          const int gstart = p_gs + 1 > p_ge + 1 - AFFIXES_LENGTH ? p_gs + 1 : p_ge + 1 - AFFIXES_LENGTH;
          const int gend = n_ge < n_gs + AFFIXES_LENGTH ? n_ge : n_gs + AFFIXES_LENGTH;
          const int gpreflen = p_ge + 1 - gstart, gsufflen = gend - n_gs, allglen = gend - gstart;
          // the three edit distances (:990, :1012, :1017): 0 without a DP where the strings are equal
          const bool there2 = estart >= esufflen && gstart >= gsufflen;
          const uint8_t* const a0 = est + c_es; const uint8_t* const b0 = T + c_gs;
          const uint8_t* const a1 = est + estart; const uint8_t* const b1 = T + gstart;
          const uint8_t* const a2 = there2 ? est + (estart - esufflen) : est; const uint8_t* const b2 = there2 ? T + (gstart - gsufflen) : T;
          bool same0 = elen == glen, same1 = epreflen == gpreflen, same2 = esufflen == gsufflen;
          if (same0) for (int x = (int)lane; x < elen; x += 64) same0 = same0 && a0[x] == b0[x];
          if (same1) for (int x = (int)lane; x < epreflen; x += 64) same1 = same1 && a1[x] == b1[x];
          if (there2 && same2) for (int x = (int)lane; x < esufflen; x += 64) same2 = same2 && a2[x] == b2[x];
          const bool run0 = !__all(same0), run1 = !__all(same1), run2 = there2 && !__all(same2);
          refused = (uint32_t)allelen > MAX_WINDOW || (run0 && (uint32_t)glen > MAX_SMALL_GEN);
          if (refused) break;
          uint32_t max_errs = 0;
          for (int k = 0; k < 3; ++k) {
            if (!(k == 0 ? run0 : k == 1 ? run1 : run2)) continue;
            DevJob job;
            job.a = k == 0 ? a0 : k == 1 ? a1 : a2; job.la = (uint32_t)(k == 0 ? elen : k == 1 ? epreflen : esufflen);
            job.b = k == 0 ? b0 : k == 1 ? b1 : b2; job.lb = (uint32_t)(k == 0 ? glen : k == 1 ? gpreflen : gsufflen);
            job.p0 = job.p1 = job.p2 = job.tail = 0;
            job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 2;
            __syncthreads();                                   // the answer before has been read
            lev_wave_body<2, MODE_ED>(job, &S.res, nullptr, lane);
            __syncthreads();
            max_errs += (uint32_t)uni(S.res.v[0]);
          }
          DevJob job;
          job.a = est + estart; job.la = (uint32_t)allelen;
          job.b = T + gstart; job.lb = (uint32_t)allglen;
          job.p0 = 0; job.p1 = (uint32_t)allelen; job.p2 = max_errs;
          job.tail = gl - (uint32_t)gend >= 2u ? 2u : gl - (uint32_t)gend;
          job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = 2;
          __syncthreads();
          lev_wave_body<2, MODE_BORDERS>(job, &S.res, nullptr, lane, S.rowmin);
          __syncthreads();
          if (uni(S.res.v[0])) {
            const int off_p = uni(S.res.v[1]), off_t1 = uni(S.res.v[2]), off_t2 = uni(S.res.v[3]);
            const int old2 = burset_adaptor(T, gl, (uint32_t)(p_ge + 1), (uint32_t)c_gs) + burset_adaptor(T, gl, (uint32_t)(c_ge + 1), (uint32_t)n_gs);
            const int nw = burset_adaptor(T, gl, (uint32_t)(gstart + off_t1), (uint32_t)(gstart + off_t2));
            outcome = 2 * nw >= old2 ? 3u : 2u;
            if (outcome == 3u && lane == 0) {                  // :1067-1070
              S.ex[prev].EST_end = estart + off_p - 1;
              S.ex[next].EST_start = eend + off_p - allelen;
              S.ex[prev].GEN_end = gstart + off_t1 - 1;
              S.ex[next].GEN_start = gend + off_t2 - allglen;
            }
          }
        }
        if (lane == 0) S.steps[curr] = (uint8_t)((S.steps[curr] & ~3u) | outcome);
        __syncthreads();
        if (outcome == 3u) {                                   // :1077-1083: curr is dropped, the merged prev is analysed again
          curr = prev;
          do { --prev; } while (prev >= 0 && (uni((int)S.steps[prev]) & 3) == 3);
          removed = true;
        }
      }
    }
    __syncthreads();
    pgpu_tail_result tr;
    tr.status = PGPU_OK; tr.verdict = (uint8_t)verdict; tr.polyA = (uint8_t)(flags & 1u); tr.polyadenil = (uint8_t)(flags >> 1);
    tr.recovered = 0; tr.n_kept = 0; tr.tail_added = added;
    if (refused) { tr.status = PGPU_ERANGE; tr.verdict = tr.polyA = tr.polyadenil = 0; tr.tail_added = 0; }
    else {
      const bool gone = verdict == 0 && lane < ne && (S.steps[lane] & 3u) == 3u;
      const uint32_t n_gone = (uint32_t)__popcll(__ballot(gone));
      if (verdict == 0) { tr.n_kept = ne - n_gone; tr.recovered = (uint8_t)recovered; }
      if (lane < ne) {
        out_exons[q.first_exon + lane] = S.ex[lane];
        uint8_t s = 0;
        if (verdict == 0) s = (uint8_t)(S.steps[lane] | (added && lane == ne - 1 ? STEP_TAIL : 0));
        out_steps[q.first_exon + lane] = s;
      }
    }
    if (lane == 0) out[c] = tr;
  }
}

}  // namespace tail_stage
