// The small stage's kernel (pgpu_index_small_chains, include/pintron_gpu.h) as a wave runs it, for the kernels that differ
// only in the longest pattern of step 1's border refinement: small_kernel (pgpu_small.hip) at R = 4 rows of the BORDERS body
// per lane, 256 rows, and small_wide_kernel (pgpu_small_wide.hip) at R = 16, 1024.  The LDS of a wave follows from R: the four
// row-minimum arrays hold 64 * R + 1 words each.  Every other cap is the same at every R.  Each dynamic program keeps its
// call sites.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_lcf.h"
#include "pgpu_classify.h"
#include "pgpu_clean_body.h"

namespace small_stage {

constexpr uint32_t MAX_EXONS = PGPU_SMALL_MAX_EXONS;
constexpr uint32_t MAX_LIST = 2 * MAX_EXONS;
constexpr uint32_t MAX_KBAND = PGPU_SMALL_MAX_KBAND;
constexpr uint32_t LB_SMALL = 6, UB_SMALL = 23, MIN_BORDER = 6;      // _LB_SMALL_EXON_LENGTH_, _UB_..., _MIN_PERFECT_BORDER_LENGTH_
static_assert(MAX_EXONS == 64, "one lane per exon of the input");
static_assert(UB_SMALL <= 64 && 2 * UB_SMALL <= 64, "lev_wave_body<1, ED> and one lane per byte of the prefix piece");
static_assert(2 * MAX_KBAND + 1 <= 64, "kband_band_sweep: the band on the lanes");

constexpr uint8_t STEP_PREFIX = 0x01, STEP_BETWEEN = 0x02, STEP_MOVED = 0x04, STEP_NOISY = 0x10, STEP_EXTERNAL = 0x20;
enum { REF_EXONS = 1, REF_WINDOW = 2, REF_LCF = 3, REF_KBAND = 4, REF_ORDER = 5 };

// the cap of the prefix's border refinement at R rows per lane
template <int R> constexpr uint32_t small_max_window() { return 64u * R; }
static_assert(small_max_window<4>() == PGPU_SMALL_MAX_PREFIX_WINDOW, "the narrow kernel's window");

template <int R>
struct SmallLds {
  pgpu_factor ex[MAX_LIST];                            // the list as the steps leave it
  uint32_t rowmin[4 * (small_max_window<R>() + 1)];    // pre, pre_pos, suf, suf_pos of the prefix's border refinement
  DevResult res;                                       // the answer of the DP at hand
  uint8_t steps[MAX_LIST];
  uint8_t piece[64];                                   // the discarded prefix's last bytes, its one N replaced
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

__device__ __forceinline__ DevJob plain_job(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, uint32_t r_class) {
  DevJob job;
  job.a = a; job.la = la; job.b = b; job.lb = lb;
  job.p0 = job.p1 = job.p2 = job.tail = 0;
  job.ws_off = 0; job.str_off = 0; job.out_idx = 0; job.r_class = r_class;
  return job;
}

// whether two pieces of `len` <= 64 bytes are equal (compute_edit_distance, src/compute-alignments.c:240-249, is 0 then
// without a dynamic program)
__device__ __forceinline__ bool same_piece(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint32_t len, uint32_t lane) {
  return __all(lane >= len || a[lane] == b[lane]);
}

// the best-run rule (best_run of pgpu_clean_body.h) over a list of up to 128 exons: the flags in two words
__device__ __forceinline__ void best_run_wide(const pgpu_factor* ex, unsigned long long bad_lo, unsigned long long bad_hi,
                                              uint32_t& lo, uint32_t& hi) {
  if (!bad_hi) { best_run(ex, bad_lo, lo, hi); return; }
  int best_cover = -1;
  uint32_t best_lo = 0, best_hi = 0, left = lo;
  for (uint32_t half = 0; half < 2; ++half) {
    unsigned long long bad = half ? bad_hi : bad_lo;
    while (bad) {
      const uint32_t r = 64u * half + (uint32_t)__builtin_ctzll(bad);
      bad &= bad - 1ull;
      if (left < r) {
        const int cover = ex[r - 1].EST_end - ex[left].EST_start + 1;
        if (cover > best_cover) { best_cover = cover; best_lo = left; best_hi = r; }
      }
      left = r + 1;
    }
  }
  if (left < hi) {
    const int cover = ex[hi - 1].EST_end - ex[left].EST_start + 1;
    if (cover > best_cover) { best_cover = cover; best_lo = left; best_hi = hi; }
  }
  lo = best_lo; hi = best_hi;
}

// The whole kernel: one wave per workgroup, a wave that has finished a query takes the next one of its stride.  Every step
// from the input; the answer to out[c], the list and the step bytes to the two slots per exon of its range.  AGAIN: the wave
// takes only the queries a kernel before it over the same arrays refused for the window (refused == 2), and leaves the
// others as they are.
template <int R, bool AGAIN>
__device__ __forceinline__ void small_body(const LcfIndexView ix, const ClassView cv, const uint8_t* __restrict__ ests,
                                           const pgpu_factor* __restrict__ exons, const pgpu_small_query* __restrict__ queries,
                                           uint32_t n_queries, const int min_intron_length, pgpu_factor* __restrict__ out_exons,
                                           uint8_t* __restrict__ out_steps, pgpu_small_result* __restrict__ out) {
  constexpr uint32_t MAX_WINDOW = small_max_window<R>();
  __shared__ SmallLds<R> S;
  const uint32_t lane = threadIdx.x;
  const uint8_t* __restrict__ T = ix.T;
  const uint32_t gl = ix.n;
  for (uint32_t c = blockIdx.x; c < n_queries; c += gridDim.x) {
    if constexpr (AGAIN) { if (uni((int)out[c].refused) != REF_WINDOW) continue; }
    const pgpu_small_query q = queries[c];
    const uint8_t* const est = ests + q.est_off;
    const uint8_t* const orig = ests + q.orig_off;
    const uint32_t ne = q.n_exons;
    uint32_t refused = ne > MAX_EXONS ? REF_EXONS : 0u;
    pgpu_factor mine;
    mine.EST_start = mine.EST_end = mine.GEN_start = mine.GEN_end = 0;
    __syncthreads();                                           // the query before is done with the LDS
    if (!refused && lane < ne) mine = exons[q.first_exon + lane];
    S.steps[lane] = 0; S.steps[lane + 64] = 0;
    // ---- what the reference asserts (:512-513, :655-658) and the tail stage's step 5 can break: refused
    {
      const int nes = __shfl_down(mine.EST_start, 1), ngs = __shfl_down(mine.GEN_start, 1);
      bool bad = false;
      if (!refused && lane < ne) {
        bad = mine.EST_start > mine.EST_end || mine.GEN_start > mine.GEN_end;
        if (lane + 1 < ne) bad = bad || mine.EST_end >= nes || mine.GEN_end >= ngs;
      }
      if (__any(bad)) refused = REF_ORDER;
    }
    uint32_t nl = 0, prefix_added = 0, verdict = 0, lo = 0, hi = 0;
    if (!refused) {
      // the exon at hand: the first of the input
      int c_es = uni(mine.EST_start), c_ee = uni(mine.EST_end), c_gs = uni(mine.GEN_start), c_ge = uni(mine.GEN_end);
      uint32_t c_steps = 0;
      // ---- step 1, search_small_exon_at_prefix (:500-606)
      if (c_es > (int)LB_SMALL) {
        const uint32_t e1len = (uint32_t)(c_ee + 1 - c_es), g1len = (uint32_t)(c_ge + 1 - c_gs);
        if (e1len + (uint32_t)c_es >= LB_SMALL + UB_SMALL) {
          const uint32_t eplen = min3u((uint32_t)c_es, (uint32_t)c_gs, 2u * UB_SMALL);
          const uint8_t* const epfact = est + ((uint32_t)c_es - eplen);
          unsigned long long key = 0ull;
          if (eplen) {                                           // (an empty piece has no common factor)
            const uint32_t ch = lane < eplen ? (uint32_t)epfact[lane] : (uint32_t)'A';
            const bool wild = ch == 'N' || ch == 'n';
            const bool acgt = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
            const unsigned long long wilds = __ballot(wild);
            if ((uint32_t)c_gs > ix.first_bad || __any(!acgt && !wild) || __popcll(wilds) > 1) refused = REF_LCF;
            else {
              // Ns_ALWAYS_MATCH_FOR_LCS: the four strings with A, C, G, T in the N's place (lcfsa_wave_body)
              const uint32_t at = wilds ? (uint32_t)__builtin_ctzll(wilds) : 0u;
              S.piece[lane] = (uint8_t)ch;
              for (uint32_t k = 0; k < (wilds ? 4u : 1u); ++k) {
                if (wilds && lane == 0) S.piece[at] = (uint8_t)"ACGT"[k];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const unsigned long long w = lcfsa_wave_key((uint32_t)c_gs, S.piece, eplen, ix, lane);
                key = w > key ? w : key;
                __builtin_amdgcn_wave_barrier();
              }
            }
          }
          const uint32_t cflen = (uint32_t)(key >> 40);
          const uint32_t pg = key ? 0x0FFFFFFFu - (uint32_t)((key >> 8) & 0x0FFFFFFFu) : 0u;
          const uint32_t pe = key ? 63u - (uint32_t)(key & 63u) : 0u;
          if (!refused && cflen >= LB_SMALL) {
            const uint32_t e1plen = min3u(e1len, g1len, UB_SMALL);
            uint32_t edp = 0;
            if (!same_piece(est + c_es, T + c_gs, e1plen, lane)) {
              const DevJob job = plain_job(est + c_es, e1plen, T + c_gs, e1plen, 1);
              __syncthreads();
              lev_wave_body<1, MODE_ED>(job, &S.res, nullptr, lane);
              __syncthreads();
              edp = (uint32_t)uni(S.res.v[0]);
            }
            // `pe` is an offset inside the piece and an absolute EST coordinate from here on, as in the reference
            const uint32_t allelen = min((uint32_t)c_ee + 1u, (uint32_t)c_es + UB_SMALL) - pe;
            const uint32_t allglen = min((uint32_t)c_ge + 1u, (uint32_t)c_gs + UB_SMALL) - pg;
            if (allelen >= 2u * LB_SMALL) {
              if (allelen > MAX_WINDOW) refused = REF_WINDOW;
              else {
                DevJob job = plain_job(est + pe, allelen, T + pg, allglen, R);
                job.p0 = LB_SMALL; job.p1 = allelen - LB_SMALL; job.p2 = edp;
                job.tail = gl - (pg + allglen) >= 2u ? 2u : gl - (pg + allglen);
                __syncthreads();
                lev_wave_body<R, MODE_BORDERS>(job, &S.res, nullptr, lane, S.rowmin);
                __syncthreads();
                if (uni(S.res.v[0])) {
                  const uint32_t off_p = (uint32_t)uni(S.res.v[1]), off_t1 = (uint32_t)uni(S.res.v[2]), off_t2 = (uint32_t)uni(S.res.v[3]);
                  bool take = (int)off_t2 - (int)off_t1 >= min_intron_length;
                  if (take) {                                    // is_canonical_intron (:481-494); a byte outside G is no match
                    const long long s = (long long)pg + off_t1, e = (long long)pg + off_t2 - 1;
                    take = s >= 0 && s + 1 < (long long)gl && e >= 1 && e < (long long)gl;
                    if (take) {
                      const uint8_t d0 = T[s], d1 = T[s + 1], a0 = T[e - 1], a1 = T[e];
                      take = (d0 == 'G' && d1 == 'T' && a0 == 'A' && a1 == 'G') || (d0 == 'g' && d1 == 't' && a0 == 'a' && a1 == 'g');
                    }
                  }
                  if (take && off_p - pe >= LB_SMALL) {          // unsigned, as in the reference
                    if (lane == 0) {
                      pgpu_factor nw;
                      nw.EST_start = (int)pe; nw.EST_end = (int)(pe + off_p) - 1; nw.GEN_start = (int)pg; nw.GEN_end = (int)(pg + off_t1) - 1;
                      S.ex[0] = nw; S.steps[0] = STEP_PREFIX;
                    }
                    nl = 1; prefix_added = 1;
                    c_es = (int)(pe + off_p); c_gs = (int)(pg + off_t2); c_steps = STEP_MOVED;
                  }
                }
              }
            }
          }
        }
      }
      // ---- step 2, search_small_exon (:641-871) for (cur, the next exon of the input); the new exon is never looked at
      for (uint32_t k = 1; k < ne && !refused; ++k) {
        int n_es = __builtin_amdgcn_readlane(mine.EST_start, (int)k), n_ee = __builtin_amdgcn_readlane(mine.EST_end, (int)k);
        int n_gs = __builtin_amdgcn_readlane(mine.GEN_start, (int)k), n_ge = __builtin_amdgcn_readlane(mine.GEN_end, (int)k);
        uint32_t n_steps = 0;
        const uint32_t e1len = (uint32_t)(c_ee + 1 - c_es), g1len = (uint32_t)(c_ge + 1 - c_gs);
        const uint32_t e2len = (uint32_t)(n_ee + 1 - n_es), g2len = (uint32_t)(n_ge + 1 - n_gs);
        unsigned long long found = 0ull;
        uint32_t estart = 0, allgstart = 0, allglen_u = 0, elen_u = 0;
        if (e1len + e2len >= LB_SMALL + 2u * UB_SMALL) {
          const uint32_t e1slen = min3u(e1len, g1len, UB_SMALL), e2plen = min3u(e2len, g2len, UB_SMALL);
          const uint32_t e1sstart = (uint32_t)c_ee + 1u - e1slen, g1sstart = (uint32_t)c_ge + 1u - e1slen;
          const uint32_t e2pstart = (uint32_t)n_es, g2pstart = (uint32_t)n_gs;
          uint32_t sed = 0, ped = 0;
          for (uint32_t side = 0; side < 2; ++side) {            // sed, ped
            const uint8_t* const a = est + (side ? e2pstart : e1sstart);
            const uint8_t* const b = T + (side ? g2pstart : g1sstart);
            const uint32_t len = side ? e2plen : e1slen;
            if (!same_piece(a, b, len, lane)) {
              const DevJob job = plain_job(a, len, b, len, 1);
              __syncthreads();
              lev_wave_body<1, MODE_ED>(job, &S.res, nullptr, lane);
              __syncthreads();
              const uint32_t d = (uint32_t)uni(S.res.v[0]);
              if (side) ped = d; else sed = d;
            }
          }
          const uint32_t cls = (uint32_t)uni((int)classify_intron(cv, (uint32_t)(c_ge + 1), (uint32_t)(n_gs - 1)));
          if (sed + ped > 2u || cls == 2u) {
            uint32_t f1slen = e1slen, f2plen = e2plen, e1socc = 0, g1socc = 0, e2pocc = 0, g2pocc = 0;
            for (uint32_t side = 0; side < 2; ++side) {          // the perfect borders of a side that is not identical
              if ((side ? ped : sed) == 0u) continue;
              const DevJob job = plain_job(est + (side ? e2pstart : e1sstart), side ? e2plen : e1slen,
                                           T + (side ? g2pstart : g1sstart), side ? e2plen : e1slen, 1);
              __syncthreads();
              lcf_small_wave_body(job, &S.res, lane);
              __syncthreads();
              const uint32_t fl = (uint32_t)uni(S.res.v[0]), eo = (uint32_t)uni(S.res.v[1]), go = (uint32_t)uni(S.res.v[2]);
              if (side) { f2plen = fl; e2pocc = eo; g2pocc = go; } else { f1slen = fl; e1socc = eo; g1socc = go; }
            }
            if (f1slen == e1slen && e2pocc > 0u) {               // :725-737, the EST byte does not move
              uint32_t nf = f1slen + 1u;
              while (nf - f1slen < e2pocc && est[e1sstart + e1socc + f1slen] == T[g2pstart + nf - f1slen]) ++nf;
              if (nf - 1u > f1slen) f1slen = nf - 1u;
            }
            // signed: where the reference's unsigned lengths would wrap (an exon shorter than a border) nothing is found
            const int elen = (int)(e1slen - e1socc) + (int)(e2pocc + f2plen) - 2 * (int)MIN_BORDER;
            estart = e1sstart + e1socc + MIN_BORDER;
            allgstart = g1sstart + g1socc + MIN_BORDER;
            const long long allglen = (long long)g2pstart + g2pocc + f2plen - MIN_BORDER - (long long)allgstart;
            const uint32_t mil = min_intron_length > 4 ? (uint32_t)min_intron_length : 4u;
            // (allgstart + allglen = g2pstart + g2pocc + f2plen - 6 ends inside the second exon, whose coordinates the entry has
            // checked: the last test cannot fail for a query that got here, and keeps sexon_search's precondition in sight)
            if (elen >= (int)LB_SMALL && elen <= (int)SEXON_MAX_ELEN && allglen > 0 && (long long)allgstart + allglen <= (long long)gl) {
              elen_u = (uint32_t)elen; allglen_u = (uint32_t)allglen;
              found = sexon_search(ix, cv, est + estart, elen_u, allgstart, allglen_u, f1slen, f2plen, mil, lane);
            }
          }
        }
        if (found && sexon_key_len(found) >= LB_SMALL) {         // :836-866
          const uint32_t len = sexon_key_len(found), os = sexon_key_offstart(found), occ = sexon_key_occ(found);
          const uint32_t oe = elen_u - os - len;
          c_ee = (int)(estart + os) - 1; c_ge = (int)(allgstart + os) - 1; c_steps |= STEP_MOVED;
          n_es = (int)(estart + os + len); n_gs = (int)(allgstart + allglen_u - oe); n_steps = STEP_MOVED;
          if (lane == 0) {
            pgpu_factor cur, nw;
            cur.EST_start = c_es; cur.EST_end = c_ee; cur.GEN_start = c_gs; cur.GEN_end = c_ge;
            nw.EST_start = (int)(estart + os); nw.EST_end = (int)(estart + os + len) - 1; nw.GEN_start = (int)occ; nw.GEN_end = (int)(occ + len) - 1;
            S.ex[nl] = cur; S.steps[nl] = (uint8_t)c_steps;
            S.ex[nl + 1] = nw; S.steps[nl + 1] = STEP_BETWEEN;
          }
          nl += 2;
        } else {
          if (lane == 0) {
            pgpu_factor cur;
            cur.EST_start = c_es; cur.EST_end = c_ee; cur.GEN_start = c_gs; cur.GEN_end = c_ge;
            S.ex[nl] = cur; S.steps[nl] = (uint8_t)c_steps;
          }
          nl += 1;
        }
        c_es = n_es; c_ee = n_ee; c_gs = n_gs; c_ge = n_ge; c_steps = n_steps;
      }
      if (!refused && lane == 0) {
        pgpu_factor cur;
        cur.EST_start = c_es; cur.EST_end = c_ee; cur.GEN_start = c_gs; cur.GEN_end = c_ge;
        S.ex[nl] = cur; S.steps[nl] = (uint8_t)c_steps;
      }
      nl += 1;
      __syncthreads();                                           // the list, for every lane
    }
    // ---- step 3, clean_factorizations (:914-950) on the ORIGINAL sequence: clean_noisy_exons, only_internals = false ...
    if (!refused) {
      bool wide = false;
      for (uint32_t i = lane; i < nl; i += 64) {
        const pgpu_factor f = S.ex[i];
        wide = wide || (f.GEN_start <= f.GEN_end && max_edit_for_exon((uint32_t)(f.GEN_end - f.GEN_start + 1)) > MAX_KBAND);
      }
      if (__any(wide)) refused = REF_KBAND;
    }
    if (!refused) {
      lo = 0; hi = nl;
      unsigned long long bad_lo = 0ull, bad_hi = 0ull;
      for (uint32_t i = 0; i < nl; ++i) {
        const pgpu_factor f = S.ex[i];
        bool ok = false;
        if (f.GEN_start <= f.GEN_end) {
          DevJob job = plain_job(T + f.GEN_start, (uint32_t)(f.GEN_end - f.GEN_start + 1), orig + f.EST_start,
                                 f.EST_end >= f.EST_start ? (uint32_t)(f.EST_end - f.EST_start + 1) : 0u, 1);
          job.p0 = max_edit_for_exon(job.la);
          __syncthreads();                                       // the answer before has been read
          lev_wave_body<1, MODE_KBAND>(job, &S.res, nullptr, lane);
          __syncthreads();
          ok = uni(S.res.v[0]) != 0;
        }
        if (!ok) {
          if (i < 64u) bad_lo |= 1ull << i; else bad_hi |= 1ull << (i - 64u);
          if (lane == 0) S.steps[i] |= STEP_NOISY;
        }
      }
      best_run_wide(S.ex, bad_lo, bad_hi, lo, hi);
      if (lo == hi) verdict = 1;
      // ... then clean_external_exons: end 0 the head, end 1 the tail (of the run as the head left it)
      for (uint32_t end = 0; end < 2 && verdict == 0; ++end) {
        const uint32_t at = end == 0 ? lo : hi - 1;
        if (!external_exon_ok(T, gl, orig, S.ex, lo, hi, end, lane)) {
          if (lane == 0) S.steps[at] |= STEP_EXTERNAL;
          if (end == 0) ++lo; else --hi;
          if (lo == hi) verdict = 2;
        }
      }
    }
    __syncthreads();                                             // the step bytes
    pgpu_small_result sr;
    sr.status = PGPU_OK; sr.refused = 0; sr.verdict = (uint8_t)verdict; sr.prefix_added = (uint8_t)prefix_added; sr.reserved = 0;
    sr.n_added = nl - ne; sr.n_list = nl; sr.first_kept = 0; sr.n_kept = 0;
    const size_t at0 = 2 * (size_t)q.first_exon;
    if (refused) {
      sr.status = PGPU_ERANGE; sr.refused = (uint8_t)refused; sr.verdict = 0; sr.prefix_added = 0; sr.n_added = 0; sr.n_list = 0;
      pgpu_factor zero;
      zero.EST_start = zero.EST_end = zero.GEN_start = zero.GEN_end = 0;
      for (size_t i = lane; i < 2 * (size_t)ne; i += 64) {
        if (i < ne) out_exons[at0 + i] = exons[q.first_exon + i]; else out_exons[at0 + i] = zero;
        out_steps[at0 + i] = 0;
      }
    } else {
      if (verdict == 0) { sr.first_kept = lo; sr.n_kept = hi - lo; }
      pgpu_factor zero;
      zero.EST_start = zero.EST_end = zero.GEN_start = zero.GEN_end = 0;
      for (uint32_t i = lane; i < 2 * ne; i += 64) {
        if (i < nl) out_exons[at0 + i] = S.ex[i]; else out_exons[at0 + i] = zero;
        out_steps[at0 + i] = i < nl ? S.steps[i] : (uint8_t)0;
      }
    }
    if (lane == 0) out[c] = sr;
  }
}

}  // namespace small_stage
