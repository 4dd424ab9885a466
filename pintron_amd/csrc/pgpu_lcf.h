// find_longest_common_factor_dp (src/factorization-refinement.c:255-316) by one wave, in its two forms: from the suffix
// array of the resident index (the whole genomic prefix against at most 46 characters of an EST) and as a diagonal sweep
// over two short strings.  The device routines dp_batch_kernel (pgpu_dp_kernels.hip) answers its KF_LCFSA and KF_LCFW jobs
// with, kept in a header so that a per-EST logic kernel (pgpu_small.hip) asks the same questions without leaving the
// device.
#pragma once
#include "pgpu_internal.h"
#include "pgpu_wave_dp.h"

// The reference keeps the FIRST maximum in (i1,i2) scan order == among maximal runs the smallest start in s1,
// then in s2; that order is folded into a 64-bit key, larger = better.
__device__ __forceinline__ unsigned long long lcf_key(uint32_t len, uint32_t occ1, uint32_t occ2) {
  return ((unsigned long long)len << 44) | ((unsigned long long)(0x0FFFFFFFu - occ1) << 16) |
         (unsigned long long)(0xFFFFu - occ2);
}

// ---------------------------------------------------------------------------------------------
// find_longest_common_factor_dp (src/factorization-refinement.c:255-316) from the suffix array.
// The small-exon search asks for the longest common factor of the WHOLE genomic prefix T[0..G) and at most
// 46 characters of the EST (:532): 46 x G cells per call in the reference (and in lcf_kernel), two calls per
// EST -- 9 M cells each on a 200 kb gene, 46 M on a 1 Mb one.  With the index resident the question is
// 64 pattern searches: lane i2 looks for the longest prefix of s2[i2..] that occurs in T and ENDS before G,
//   l <= 8     first_occ_l[code] <= G - l          (a table of first occurrences per l-mer: one probe per l,
//                                                   all eight independent of each other)
//   l  > 8     the interval of the 8-mer in the suffix array, narrowed one character at a time by bisection
//              (a handful of suffixes on a gene-sized sequence); "some occurrence ends before G" is
//              min(SA[lo..hi)) <= G - l, a range minimum read off a sparse table; as soon as one suffix is
//              left the rest is a direct comparison of the two strings.
// "Valid at l + 1" implies "valid at l", so a lane stops at its first failure.  The reference keeps the FIRST
// maximum in (i1, i2) scan order = the longest factor with the smallest start in T, then in s2: every lane
// carries the smallest start of its best length and the wave agrees on (max length, min start, min lane).
// Only exact matching is expressed this way: the library sends a job here when T[0..G) and s2 consist of
// upper-case A, C, G, T alone (no N wildcard can fire: Ns_ALWAYS_MATCH_FOR_LCS, :74), and to lcf_kernel otherwise.
// ---------------------------------------------------------------------------------------------
// find_longest_common_factor_dp of two SHORT strings (the exon ends the small-exon search compares,
// src/factorization-refinement.c:690-718: at most 23 x 23 cells; nine jobs in ten of a C3 batch): one wave,
// lane = diagonal, in rounds of 64 diagonals; N wildcard and first-maximum rule as in lcf_kernel (same key).
// These used to get a workgroup, an atomic and a host-side decode each, in a launch of their own.
__device__ __forceinline__ void lcf_small_wave_body(const DevJob& job, DevResult* res, const uint32_t lane) {
  const uint32_t l1 = job.la, l2 = job.lb;
  const uint8_t* __restrict__ s1 = job.a; const uint8_t* __restrict__ s2 = job.b;
  unsigned long long best = 0;
  if (l1 != 0 && l2 != 0) {
    const uint32_t ndiag = l1 + l2 - 1;
    for (uint32_t dg0 = 0; dg0 < ndiag; dg0 += 64) {
      const uint32_t dg = dg0 + lane;
      if (dg < ndiag) {
        // cells of this diagonal: i2 from max(0, l2-1-dg), i1 = i2 + dg - (l2-1)
        const uint32_t i2_lo = dg < l2 - 1 ? l2 - 1 - dg : 0;
        const int32_t shift = (int32_t)dg - (int32_t)(l2 - 1);
        uint32_t i2_hi = l2;
        if ((int32_t)l1 - shift < (int32_t)i2_hi) i2_hi = (uint32_t)((int32_t)l1 - shift);
        uint32_t run = 0, brun = 0, bend = 0;
        for (uint32_t i2 = i2_lo; i2 < i2_hi; ++i2) {
          const uint32_t c1 = s1[(int32_t)i2 + shift], c2 = s2[i2];
          run = (c1 == c2 || is_n(c1) || is_n(c2)) ? run + 1 : 0;
          if (run > brun) { brun = run; bend = i2; }
        }
        if (brun > 0) {
          const uint32_t occ2 = bend + 1 - brun;
          const unsigned long long key = lcf_key(brun, (uint32_t)((int32_t)occ2 + shift), occ2);
          best = key > best ? key : best;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const unsigned long long x = __shfl_xor(best, o); best = x > best ? x : best; }
  if (lane == 0) {
    res->status = 0;
    res->v[0] = (int32_t)(best >> 44);
    res->v[1] = best ? (int32_t)(0x0FFFFFFFu - (uint32_t)((best >> 16) & 0x0FFFFFFFu)) : 0;
    res->v[2] = best ? (int32_t)(0xFFFFu - (uint32_t)(best & 0xFFFFu)) : 0;
  }
}

__device__ __forceinline__ uint32_t lcfsa_rmq(const LcfIndexView& ix, uint32_t lo, uint32_t hi) {   // min(sa[lo..hi)), hi > lo
  const uint32_t len = hi - lo;
  const uint32_t j = 31u - (uint32_t)__builtin_clz(len);
  const uint32_t* lv = j == 0 ? ix.sa : ix.rmq + (size_t)(j - 1) * ix.n;
  return min(lv[lo], lv[hi - (1u << j)]);
}

// the search for one string s2 of upper-case A, C, G, T: the wave's key (longest, then smallest start in T, then
// smallest start in s2), the same in every lane; 0 = no common factor
__device__ __forceinline__ unsigned long long lcfsa_wave_key(const uint32_t G, const uint8_t* s2, const uint32_t l2,
                                                             const LcfIndexView& ix, const uint32_t lane) {
  const uint8_t* __restrict__ T = ix.T;
  uint32_t best = 0, bt = 0;
  if (lane < l2) {
    const uint32_t i2 = lane, r = l2 - i2, lim = min(r, 8u);
    uint32_t fo[8], code = 0, off = 0, width = 4;
#pragma unroll
    for (uint32_t l = 1; l <= 8; ++l) {                      // eight independent probes
      fo[l - 1] = 0xFFFFFFFFu;
      if (l <= lim) {
        const int b = acgt_code(s2[i2 + l - 1]);
        code = code * 4u + (uint32_t)(b < 0 ? 0 : b);
        fo[l - 1] = ix.focc[off + code];
      }
      off += width; width *= 4u;
    }
    bool ok = true;
#pragma unroll
    for (uint32_t l = 1; l <= 8; ++l) {
      if (ok && l <= lim && l <= G && fo[l - 1] <= G - l) { best = l; bt = fo[l - 1]; }
      else ok = false;
    }
    if (best == 8 && r > 8) {
      uint32_t lo = ix.klo[code], hi = ix.khi[code], l = 8;
      while (l < r && hi > lo) {
        if (hi - lo == 1) {
          // one suffix left: lengths l+1 .. min(lcp, G - t) are valid with this start
          const uint32_t t = ix.sa[lo], cap = min(r, G - t);
          uint32_t m = l;
          while (m < cap) {
            // eight characters of each side per round trip
            uint32_t eq = 0;
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) {
              const bool in = m + q < cap;
              const uint32_t a = in ? T[t + m + q] : 0u, b = in ? s2[i2 + m + q] : 1u;
              eq |= (a == b ? 1u : 0u) << q;
            }
            const uint32_t run = (uint32_t)__builtin_ctz(~eq);      // matching characters from m on (at most 8)
            m += run;
            if (run < 8) break;
          }
          if (m > best) { best = m; bt = t; }
          break;
        }
        const uint32_t c = s2[i2 + l];
        // suffixes of [lo, hi) share l characters and are ordered by the next one (the end of T first)
        uint32_t a = lo, z = hi;
        while (a < z) { const uint32_t mid = (a + z) >> 1, p = ix.sa[mid] + l; const uint32_t ch = p < ix.n ? T[p] : 0u; if (ch < c) a = mid + 1; else z = mid; }
        const uint32_t nlo = a;
        z = hi;
        while (a < z) { const uint32_t mid = (a + z) >> 1, p = ix.sa[mid] + l; const uint32_t ch = p < ix.n ? T[p] : 0u; if (ch <= c) a = mid + 1; else z = mid; }
        lo = nlo; hi = a;
        if (lo == hi) break;
        ++l;
        const uint32_t mt = lcfsa_rmq(ix, lo, hi);
        if (l <= G && mt <= G - l) { best = l; bt = mt; } else break;
      }
    }
  }
  // the wave's answer: longest, then smallest start in T, then smallest start in s2 (= lane)
  unsigned long long key = best ? ((unsigned long long)best << 40) | ((unsigned long long)(0x0FFFFFFFu - bt) << 8) | (63u - lane) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const unsigned long long x = __shfl_xor(key, o); key = x > key ? x : key; }
  return key;
}

// job.p0 = 0: s2 is upper-case ACGT.  job.p0 = q + 1: s2[q] is an N, the only character of s2 that is not ACGT.
// Ns_ALWAYS_MATCH_FOR_LCS (src/factorization-refinement.c:74) makes that N equal to whatever the genomic sequence
// holds there; the genomic prefix is ACGT only (the host checked), so the factors that run over the N are the exact
// factors of the four strings s2 with A, C, G, T in its place, and the reference's first maximum -- longest, then
// smallest start in T, then in s2 -- is the largest of the four keys.  `scratch`: 64 bytes of the wave's LDS.
__device__ __forceinline__ void lcfsa_wave_body(const DevJob& job, DevResult* res, const LcfIndexView& ix, const uint32_t lane,
                                                uint8_t* scratch) {
  const uint32_t G = job.la, l2 = job.lb;
  unsigned long long key;
  if (job.p0 == 0u) key = lcfsa_wave_key(G, job.b, l2, ix, lane);
  else {
    key = 0ull;
    const uint32_t q = job.p0 - 1u;
    if (lane < l2) scratch[lane] = job.b[lane];
    for (uint32_t c = 0; c < 4u; ++c) {
      if (lane == 0) scratch[q] = (uint8_t)"ACGT"[c];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const unsigned long long k = lcfsa_wave_key(G, scratch, l2, ix, lane);
      key = k > key ? k : key;
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (lane == 0) {
    res->status = 0;
    res->v[0] = (int32_t)(key >> 40);
    res->v[1] = key ? (int32_t)(0x0FFFFFFFu - (uint32_t)((key >> 8) & 0x0FFFFFFFu)) : 0;
    res->v[2] = key ? (int32_t)(63u - (uint32_t)(key & 63u)) : 0;
  }
}
