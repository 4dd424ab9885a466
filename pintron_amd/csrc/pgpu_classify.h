// Class of an intron (U12 / U2 / not classified) from the classification tables of the resident index, and the
// search loop of search_small_exon (src/factorization-refinement.c:772-834) over them: the device routines the
// kernels of pgpu_classify.hip are made of, kept in a header so that a per-EST logic kernel can ask both questions
// without leaving the device (as pgpu_find.h).
//
// The tables (built by class_tables_kernel, pgpu_classify.hip), n = length of the sequence, n + 1 entries each:
//   cls_start[s]  bits 0-1  kind of T[s], T[s+1]: 1 GT, 2 GC, 3 AT (either case), 0 anything else or s + 1 >= n
//                 bits 2-3  outcome of the score comparisons the kind selects when the intron's end agrees
//                           (GT..AG, GC..AG, AT..AC): bit 0 of the pair u12 > u2, bit 1 u12 - u2 > 0.25 && u12 >= 0.75
//                 bits 4-5  the same two outcomes for the general case (best U12 matrix against best U2 matrix)
//                 bit 7     set (filled)
//   cls_end[e]    for an intron whose LAST byte is T[e]: bits 0-1 kind of T[e-1], T[e]: 1 AG, 2 AC, 0 otherwise;
//                 bit 2 a branch point is found for an intron that ends here and is at least 30 long; bit 7 filled
// This is the layout of cls_start[] / cls_end[] of pintron_amd/host/ef_classify.c:168-216; unlike there, bits 4-5 are
// filled at every position up to n, so that every (start, end) is answered from the tables.
#pragma once
#include "pgpu_find.h"

struct ClassView { const uint8_t* cls_start; const uint8_t* cls_end; uint32_t n; };
// The view of an index's tables for a kernel of another file (pgpu_classify.hip): they are built now, on the context's
// bound device and stream, when nobody has asked before.  PGPU_OK, or the failed context's code.
int pgpu_class_view_get(pgpu_ctx* ctx, const pgpu_index* idx, ClassView* out);

enum { CLS_P5_GT = 1, CLS_P5_GC = 2, CLS_P5_AT = 3, CLS_P3_AG = 1, CLS_P3_AC = 2 };

// classify_genomic_intron_start_end (src/classify-intron.c:95-229), class only: 0 U12, 1 U2, 2 not classified, of
// the intron T[start .. end], both inclusive.  The intron is cut at the end of the sequence (real_substring stops
// at the terminator); end < start or start >= n is the empty intron.
__device__ __forceinline__ uint32_t classify_intron(const ClassView& cv, uint32_t start, uint32_t end) {
  uint32_t il = 0;                                  // bytes of the intron inside the sequence
  if (start < cv.n && end >= start) {
    const uint32_t room = cv.n - start;
    il = end - start >= room ? room : end - start + 1;
  }
  const uint32_t cs = cv.cls_start[start < cv.n ? start : cv.n];
  const uint32_t ce = il >= 2 ? cv.cls_end[start + il - 1] : 0u;      // below two bytes neither dinucleotide exists
  const uint32_t p5 = il >= 2 ? cs & 3u : 0u, p3 = ce & 3u;
  const bool own = (p5 == CLS_P5_GT && p3 == CLS_P3_AG) || (p5 == CLS_P5_GC && p3 == CLS_P3_AG) ||
                   (p5 == CLS_P5_AT && p3 == CLS_P3_AC);
  const uint32_t bits = own ? (cs >> 2) & 3u : (cs >> 4) & 3u;
  if (il >= 30 && (ce & 4u)) return (bits & 1u) ? 0u : 1u;            // branch point: u12 > u2 ? U12 : U2
  if (own && p5 != CLS_P5_AT) return 1u;                              // GT..AG / GC..AG without one: U2
  return (bits & 2u) ? 0u : 2u;
}

// ---- the small-exon search -------------------------------------------------------------------------------------
// Candidates are ordered by a packed key, larger = better: length, then smaller offstart, then smaller occurrence
// (the reference replaces its best on strictly greater length only, :816, so the first candidate of the maximal
// length in loop order wins).  0: no candidate.
constexpr uint32_t SEXON_MAX_ELEN = 64;             // PGPU_SEXON_MAX_ELEN
__device__ __forceinline__ unsigned long long sexon_key(uint32_t len, uint32_t offstart, uint32_t occ) {
  return ((unsigned long long)len << 40) | ((unsigned long long)(0xFFu - offstart) << 32) | (0xFFFFFFFFu - occ);
}
__device__ __forceinline__ uint32_t sexon_key_len(unsigned long long k) { return (uint32_t)(k >> 40); }
__device__ __forceinline__ uint32_t sexon_key_offstart(unsigned long long k) { return 0xFFu - (uint32_t)((k >> 32) & 0xFFu); }
__device__ __forceinline__ uint32_t sexon_key_occ(unsigned long long k) { return 0xFFFFFFFFu - (uint32_t)k; }

__device__ __forceinline__ unsigned long long sexon_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t sexon_min3(uint32_t a, uint32_t b, uint32_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

// One lane's occurrence `occ` of the shortest pattern of this offstart: how far the match goes on, the class of the
// first intron (which does not depend on offend), then the offends from the longest pattern that still matches
// down; the first whose second intron is classified is the best this occurrence can give.  Patterns not longer
// than `floor_len` cannot win any more and are not looked at.
__device__ __forceinline__ unsigned long long sexon_eval(const uint8_t* __restrict__ T, const ClassView& cv, const uint8_t* __restrict__ P,
                                                         uint32_t occ, uint32_t pmin, uint32_t rem, uint32_t max_offend,
                                                         uint32_t i1start, uint32_t gend, uint32_t offstart, uint32_t floor_len) {
  uint32_t ext = pmin;                              // occ + rem <= n: the caller's window
  while (ext < rem && T[occ + ext] == P[ext]) ++ext;
  if (ext <= floor_len) return 0ull;
  if (classify_intron(cv, i1start, occ - 1) == 2u) return 0ull;
  for (uint32_t offend = rem - ext; offend < max_offend; ++offend) {
    const uint32_t plen = rem - offend;
    if (plen <= floor_len) break;
    if (classify_intron(cv, occ + plen, gend - offend - 1) != 2u) return sexon_key(plen, offstart, occ);
  }
  return 0ull;
}

// The loop of search_small_exon (:772-834) for one query, by all 64 lanes of a wave with the same arguments; the
// same key in every lane.  E = efact (elen <= SEXON_MAX_ELEN bytes), the caller has checked allgstart + allglen <= n
// and min_intron_len >= 4.  All patterns of one offstart begin at E + offstart and the occurrences of a longer one
// are among those of the shortest, so per offstart: the suffix-array interval of the shortest pattern (or the
// window's positions when they are fewer), one lane per occurrence.  The window of an occurrence does not depend on
// offend: occ >= allgstart + offstart + MIL and occ + (elen - offstart) <= allgstart + allglen - MIL.
__device__ __forceinline__ unsigned long long sexon_search(const LcfIndexView& ix, const ClassView& cv, const uint8_t* __restrict__ E,
                                                           uint32_t elen, uint32_t allgstart, uint32_t allglen, uint32_t f1slen,
                                                           uint32_t f2plen, uint32_t mil, uint32_t lane) {
  // the four gates of :743-758 (2 * MIL + 6 in 64 bits: MIL is the caller's)
  if (f1slen < 6u || f2plen < 6u || (unsigned long long)allglen < 2ull * mil + 6ull || elen < 6u) return 0ull;
  const uint32_t groom = allglen + 1u - 2u * mil - 6u;             // allglen + 1 - 2 MIL - LB of :778, >= 1
  const uint32_t max_offstart = sexon_min3(f1slen - 5u, elen - 5u, groom);
  const uint32_t gend = allgstart + allglen;
  unsigned long long best = 0ull;
  for (uint32_t offstart = 0; offstart < max_offstart; ++offstart) {
    const uint32_t rem = elen - offstart;                          // the longest pattern of this offstart
    const uint32_t floor_len = sexon_key_len(best);
    if (floor_len >= rem) break;                                   // an equal length at a larger offstart loses
    const uint32_t max_offend = sexon_min3(f2plen - 5u, rem - 5u, groom - offstart);
    const uint32_t pmin = rem - (max_offend - 1u);                 // >= 6
    const uint32_t lo = allgstart + offstart + mil;
    if (allglen < 2u * mil + elen) continue;                       // no room for the longest pattern ...
    const uint32_t hi = gend - mil - rem;                          // ... else the last start, >= lo
    if (hi < lo) continue;
    const uint8_t* __restrict__ P = E + offstart;
    uint32_t a, b;
    find_sa_interval(ix, P, pmin, lane, &a, &b);
    if (a >= b) continue;
    const uint32_t width = hi - lo + 1u, i1start = allgstart + offstart;
    unsigned long long mine = 0ull;
    if (width < b - a) {                                           // fewer window positions than occurrences
      for (uint32_t base = 0; base < width; base += 64) {
        const uint32_t i = base + lane;
        if (i < width && find_match_at(ix.T, lo + i, P, pmin)) {
          const unsigned long long k = sexon_eval(ix.T, cv, P, lo + i, pmin, rem, max_offend, i1start, gend, offstart, floor_len);
          mine = k > mine ? k : mine;
        }
      }
    } else {
      for (uint32_t k0 = a; k0 < b; k0 += 64) {
        const uint32_t k = k0 + lane;
        if (k < b) {
          const uint32_t t = ix.sa[k];
          if (t >= lo && t <= hi) {
            const unsigned long long key = sexon_eval(ix.T, cv, P, t, pmin, rem, max_offend, i1start, gend, offstart, floor_len);
            mine = key > mine ? key : mine;
          }
        }
      }
    }
    const unsigned long long w = sexon_wave_max(mine);
    best = w > best ? w : best;
  }
  return best;
}
