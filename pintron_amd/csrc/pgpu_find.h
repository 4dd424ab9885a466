// Exact occurrences of a string in the resident genomic sequence: the wave-level device routines over the
// index view (pgpu_index.h).  They are what the exact-occurrence query's kernels (pgpu_find.hip) are made of,
// and are kept in a header so that a per-EST logic kernel can ask the same question without leaving the device.
//
// Matching is byte equality, what strstr / memcmp see in the reference's search_small_exon
// (src/factorization-refinement.c:781-834): case-sensitive, 'N' is a letter like any other.
//
// Every routine here is called by ALL 64 lanes of a wave with the same arguments (`lane` = the caller's lane
// index) and returns the same value in every lane.
#pragma once
#include "pgpu_index.h"

// Order of the suffix T[t..n) against P[0..len), given that the first `skip` bytes agree: -1 the suffix sorts
// before every string that starts with P, 0 P is a prefix of the suffix, +1 the suffix sorts behind.  64 bytes per
// step, one per lane, the first difference found by ballot.  The end of the text compares as "smaller than any
// byte" (the order the suffix array was built in), and nothing at or beyond T[n] is read.
__device__ __forceinline__ int find_cmp_suffix(const LcfIndexView& ix, uint32_t t, const uint8_t* __restrict__ P, uint32_t len,
                                               uint32_t skip, uint32_t lane) {
  for (uint32_t off = skip; off < len; off += 64) {
    const uint32_t j = off + lane;
    int c = 0;                                      // text byte - pattern byte at this lane's position
    if (j < len) {
      const uint32_t p = t + j;                     // t < n < 2^28 and len <= n: no wrap
      c = (p < ix.n ? (int)ix.T[p] : -1) - (int)P[j];
    }
    const unsigned long long diff = __ballot(c != 0);
    if (diff) return (__ballot(c < 0) >> __builtin_ctzll(diff)) & 1ull ? -1 : 1;
  }
  return 0;
}

// 2-bit code of P[0..KTAB) when all of them are upper-case A, C, G, T; -1 otherwise
__device__ __forceinline__ int find_kmer_code(const uint8_t* __restrict__ P) {
  int code = 0;
#pragma unroll
  for (uint32_t x = 0; x < KTAB; ++x) {
    const uint32_t c = P[x];
    const int b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
    if (b < 0) return -1;
    code = (code << 2) | b;
  }
  return code;
}

// [*lo, *hi): the suffix-array entries whose suffix starts with P[0..len), len >= 1.  A pattern of at least KTAB
// bytes that begins with an upper-case ACGT k-mer starts from that k-mer's interval and compares from byte KTAB
// on; any other pattern (shorter than KTAB, or with another byte among its first KTAB) bisects the whole array.
__device__ __forceinline__ void find_sa_interval(const LcfIndexView& ix, const uint8_t* __restrict__ P, uint32_t len, uint32_t lane,
                                                 uint32_t* lo, uint32_t* hi) {
  uint32_t from = 0, to = ix.n, skip = 0;
  if (len >= KTAB) {
    const int code = find_kmer_code(P);
    if (code >= 0) { from = ix.klo[code]; to = ix.khi[code]; skip = KTAB; }
  }
  uint32_t a = from, b = to;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (find_cmp_suffix(ix, ix.sa[mid], P, len, skip, lane) < 0) a = mid + 1; else b = mid;
  }
  *lo = a;
  b = to;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (find_cmp_suffix(ix, ix.sa[mid], P, len, skip, lane) <= 0) a = mid + 1; else b = mid;
  }
  *hi = a;
}

// one lane's own comparison: T[t .. t + len) == P[0 .. len); the caller guarantees t + len <= n
__device__ __forceinline__ bool find_match_at(const uint8_t* __restrict__ T, uint32_t t, const uint8_t* __restrict__ P, uint32_t len) {
  uint32_t j = 0;
  while (j < len && T[t + j] == P[j]) ++j;
  return j == len;
}
