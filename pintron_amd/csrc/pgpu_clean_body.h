// Two rules of the cleaning steps that more than one stage kernel applies to the exons in its LDS: the best-run rule of
// clean_low_complexity_exons_2 and clean_noisy_exons, and the test of clean_external_exons on one end exon.  clean_kernel
// (pgpu_clean.hip) runs them on a candidate, small_kernel (pgpu_small.hip) on a refined factorization over the original
// sequence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pintron_gpu.h"

// update_with_subfact_with_best_coverage (:1900-1987) on the run [lo, hi) with the exons of `bad` flagged: the run of
// unflagged exons with the largest cover on the EST, the first of equals; lo == hi when none is left
__device__ __forceinline__ void best_run(const pgpu_factor* ex, unsigned long long bad, uint32_t& lo, uint32_t& hi) {
  if (!bad) return;
  int best_cover = -1;
  uint32_t best_lo = 0, best_hi = 0, left = lo;
  while (bad) {
    const uint32_t r = (uint32_t)__builtin_ctzll(bad);
    bad &= bad - 1ull;
    if (left < r) {
      const int cover = ex[r - 1].EST_end - ex[left].EST_start + 1;
      if (cover > best_cover) { best_cover = cover; best_lo = left; best_hi = r; }
    }
    left = r + 1;
  }
  if (left < hi) {
    const int cover = ex[hi - 1].EST_end - ex[left].EST_start + 1;
    if (cover > best_cover) { best_cover = cover; best_lo = left; best_hi = hi; }
  }
  lo = best_lo; hi = best_hi;
}

// a genomic byte for the splice sites: upper case, 0 outside the sequence
__device__ __forceinline__ uint32_t splice_site_byte(const uint8_t* __restrict__ T, const uint32_t n, const int i) {
  return (i >= 0 && (uint32_t)i < n) ? ((uint32_t)T[i] & ~32u) : 0u;
}

// clean_external_exons (:1706-1825) on one end of the run [lo, hi) of `ex`: end 0 the head, end 1 the tail.  False: the
// exon is dropped.  An exon of 20 genomic bytes or more stays, one of fewer than 10 goes; between them it stays when it
// has a neighbour, the intron between them has its GT / GC .. AG, and the exon's two pieces are equal as byte strings (an
// edit distance > 0 is that they differ).  The same answer in every lane.
__device__ __forceinline__ bool external_exon_ok(const uint8_t* __restrict__ T, const uint32_t n, const uint8_t* __restrict__ est,
                                                 const pgpu_factor* ex, const uint32_t lo, const uint32_t hi, const uint32_t end,
                                                 const uint32_t lane) {
  const uint32_t at = end == 0 ? lo : hi - 1;
  const pgpu_factor f = ex[at];
  const int gl = f.GEN_end - f.GEN_start + 1, el = f.EST_end - f.EST_start + 1;
  bool ok = gl >= 10;
  if (ok && gl < 20) {
    if (hi - lo < 2) ok = false;                                       // no neighbour to share an intron with
    else if (end == 0) {
      const int acc = ex[lo + 1].GEN_start;
      ok = splice_site_byte(T, n, f.GEN_end + 1) == 'G' &&
           (splice_site_byte(T, n, f.GEN_end + 2) == 'T' || splice_site_byte(T, n, f.GEN_end + 2) == 'C') &&
           splice_site_byte(T, n, acc - 2) == 'A' && splice_site_byte(T, n, acc - 1) == 'G';
    } else {
      const int don = ex[hi - 2].GEN_end;
      ok = splice_site_byte(T, n, f.GEN_start - 2) == 'A' && splice_site_byte(T, n, f.GEN_start - 1) == 'G' &&
           splice_site_byte(T, n, don + 1) == 'G' &&
           (splice_site_byte(T, n, don + 2) == 'T' || splice_site_byte(T, n, don + 2) == 'C');
    }
    // an edit distance > 0: the two pieces differ as byte strings
    if (ok) {
      bool differ = gl != el;
      if (!differ && (int)lane < gl) differ = T[f.GEN_start + (int)lane] != est[f.EST_start + (int)lane];
      ok = !__any(differ);
    }
  }
  return ok;
}
